"""Host-side mirror of the reference's user API for the hot path (types.jl:7-269):

    LeastSquaresProblem(x=..., f_=..., g_=..., J=..., y=..., output_length=...)
    optimize_(nls, Dogleg(QR()) | LevenbergMarquardt(LSMR()) | ..., x_tol=..., lower=..., ...)
    optimize(f, x, optimizer, ...)

(`f_`/`g_`/`optimize_` stand for Julia's `f!`/`g!`/`optimize!`).  The trust-region control runs
on the host, every m-/n-/nnz-length array lives on the MI355X and every arithmetic step is a
hand-written HIP kernel reached through the C ABI of include/lsqhip.h.  The Julia side of the same
boundary is shown in INTEGRATION.md.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (ArgumentError, DimensionMismatch, check, lib)

try:  # scipy is only needed to accept csc_matrix Jacobians
    import scipy.sparse as _sp
except Exception:  # pragma: no cover
    _sp = None


# ------------------------------------------------------------------------------------------------
# solver / optimizer selectors (types.jl:76-98)
# ------------------------------------------------------------------------------------------------
class AbstractSolver:
    pass


class QR(AbstractSolver):
    kind = _lib.QR


class Cholesky(AbstractSolver):
    kind = _lib.CHOLESKY


class BlockQR(AbstractSolver):
    """QR() per block of a BlockDiagonal Jacobian (nb <= 64): column-pivoted QR of every block with its own rank decision
    (dense_qr.jl:30-88 on J_b alone) -- backward stable where Cholesky() squares the condition number, and a rank-deficient,
    all-zero or wide block gets its minimum-norm solution instead of an error.  QR() on the stacked matrix would make ONE
    rank decision; this makes one per fit."""
    kind = _lib.BLOCK_QR


class Schur(AbstractSolver):
    """Cholesky()'s damped solve on a BorderedBlockDiagonal Jacobian with ANY number of shared columns (nb <= 64;
    LevenbergMarquardt only): the locals are eliminated block by block, the border passes through in tiles of 64 columns, and
    the ng x ng Schur complement is factored by the dense Cholesky() machinery.  Same semantics as Cholesky() on that
    container -- unpivoted dpotrf on the stacked normal matrix with the locals first, PosDefException at its column."""
    kind = _lib.SCHUR


class BorderedQR(AbstractSolver):
    """The backward-stable direct solver on a BorderedBlockDiagonal Jacobian (nb <= 64, any ng; LevenbergMarquardt only): the
    damped solve as the least-squares problem min ||[J; diag(sqrt(damp))] x - [y; 0]|| by Householder reflectors.  The locals
    are eliminated block by block (unpivoted) against a triangle that starts as diag(sqrt(damp_b)), the transformed border goes
    to one dense QR() solve, then the locals are substituted back.  J'J is never formed: the error grows with cond(J) where
    Cholesky() and Schur() pay cond(J)^2.  A local column that is zero with zero damping, or a non-finite value, raises
    RankDeficientException with the stacked column; the shared part never fails on rank."""
    kind = _lib.BORDERED_QR


class LSMR(AbstractSolver):
    """LSMR(preconditioner!, P) (types.jl:82-86).

    * `LSMR(preconditioner=fn)` -- DIAGONAL preconditioners, fused into the device-resident recurrence: `fn(P, J, damp)` is
      the reference's preconditioner!(P, x, J, damp); it must fill the DeviceVector P with the factors the preconditioner
      solve multiplies by (an InverseDiagonal stores the inverse, iterative_lsmr.jl:117-122) for J'J + diag(damp); damp is a
      DeviceVector with the un-rooted damping or None (Dogleg).  The solver owns the storage P.
    * `LSMR(preconditioner=fn, P=obj)` -- ANY preconditioner that supports ldiv! (README.md:47 of the reference): `obj` is the
      caller's own object with a method `obj.ldiv(out, x)` (= ldiv!(out, P, x) on DeviceVectors); `fn(obj, J, damp)` refreshes
      it before every solve (None: P never changes).  Runs the operator-level recurrence (lsq_lsmr_general.hip): the slow
      path, as a user-supplied P is in the reference.
    Either callback runs on the host before / inside every solve.  None = the built-in Jacobi preconditioner
    (iterative_lsmr.jl:129-141)."""
    kind = _lib.LSMR

    def __init__(self, preconditioner=None, P=None):
        if P is not None and not hasattr(P, "ldiv"):
            raise TypeError("LSMR(preconditioner!, P): P must provide ldiv(out, x)  (ldiv!(out, P, x))")
        self.preconditioner = preconditioner
        self.P = P


def _general_precond_trampolines(solver, ctx, J):
    """(update_cb, ldiv_cb) for LSMR(preconditioner!, P) with a general P."""
    P, fn = solver.P, solver.preconditioner

    def _update(_jh, d_damp, _user):
        try:
            if fn is not None:
                fn(P, J, DeviceVector.borrow(ctx, J.n, d_damp) if d_damp else None)
            return 0
        except Exception as e:   # pragma: no cover
            import sys
            print("preconditioner! callback failed:", e, file=sys.stderr)
            return 1

    def _ldiv(d_out, d_in, _user):
        try:
            P.ldiv(DeviceVector.borrow(ctx, J.n, d_out), DeviceVector.borrow(ctx, J.n, d_in))
            return 0
        except Exception as e:   # pragma: no cover
            import sys
            print("preconditioner ldiv callback failed:", e, file=sys.stderr)
            return 1

    return _lib.PRECOND_UPDATE_CALLBACK(_update), _lib.PRECOND_LDIV_CALLBACK(_ldiv)


def _precond_trampoline(fn, ctx, J):
    """ctypes callback (d_P, J_handle, d_damp, user) -> fn(P, J, damp) on borrowed DeviceVector views."""
    def _cb(d_p, _jh, d_damp, _user):
        try:
            P = DeviceVector.borrow(ctx, J.n, d_p)
            damp = DeviceVector.borrow(ctx, J.n, d_damp) if d_damp else None
            fn(P, J, damp)
            return 0
        except Exception as e:   # pragma: no cover
            import sys
            print("preconditioner callback failed:", e, file=sys.stderr)
            return 1
    return _lib.PRECOND_CALLBACK(_cb)


class AbstractOptimizer:
    def __init__(self, solver=None):
        if isinstance(solver, type):
            solver = solver()
        self.solver = solver


class Dogleg(AbstractOptimizer):
    kind = _lib.DOGLEG
    name = "Dogleg"


class LevenbergMarquardt(AbstractOptimizer):
    kind = _lib.LEVENBERG_MARQUARDT
    name = "LevenbergMarquardt"


def _is_sparse(J):
    return _sp is not None and _sp.issparse(J)


class BlockDiagonal:
    """J = blkdiag(J_1 .. J_B), every block dense mb x nb: the Jacobian of B independent small fits stacked into one
    problem (m = B*mb residuals, n = B*nb parameters).  A host-side container like a scipy CSC matrix with a fixed pattern:
    `.data` is the flat value array g_ overwrites (the sparse contract, test/nonlinearleastsquares.jl:47-86), ordered
    [block][column][row] -- B column-major mb x nb blocks back to back, which IS the nzval order of `.tocsc()`.
    On the device it becomes a CSC handle that knows its block shape (lsq_blockdiag_create): LSMR() is the default solver
    (types.jl:114-127: anything not dense), Cholesky() solves the B normal-equation blocks in one pass (nb <= 64),
    BlockQR() factors every block by column-pivoted QR in one pass (nb <= 64), QR() is refused as for every sparse
    Jacobian."""

    def __init__(self, nblocks, mb, nb, data=None):
        nblocks, mb, nb = int(nblocks), int(mb), int(nb)
        if nblocks < 1 or mb < 1 or nb < 1:
            raise DimensionMismatch(_lib.EDIM, "BlockDiagonal needs nblocks >= 1, mb >= 1, nb >= 1 (got %d, %d, %d)"
                                    % (nblocks, mb, nb))
        self.nblocks, self.mb, self.nb = nblocks, mb, nb
        self.shape = (nblocks * mb, nblocks * nb)
        self.nnz = nblocks * mb * nb
        if data is None:
            self.data = np.zeros(self.nnz)
        else:
            d = np.ascontiguousarray(data, dtype=np.float64).reshape(-1)
            if d.size != self.nnz:
                raise DimensionMismatch(_lib.EDIM, "BlockDiagonal: expected %d values, got %d" % (self.nnz, d.size))
            self.data = d

    @classmethod
    def from_blocks(cls, blocks):
        """From a sequence of equally shaped (mb, nb) arrays."""
        blocks = [np.asarray(b, dtype=np.float64) for b in blocks]
        if not blocks or blocks[0].ndim != 2:
            raise DimensionMismatch(_lib.EDIM, "BlockDiagonal.from_blocks needs a non-empty sequence of matrices")
        mb, nb = blocks[0].shape
        for k, b in enumerate(blocks):
            if b.shape != (mb, nb):
                raise DimensionMismatch(_lib.EDIM, "BlockDiagonal.from_blocks: block %d is %s, block 0 is %s"
                                        % (k, b.shape, (mb, nb)))
        out = cls(len(blocks), mb, nb)
        for k, b in enumerate(blocks):
            out.block(k)[:, :] = b
        return out

    def block(self, b):
        """Block b as an (mb, nb) VIEW into `.data` (as it is bound at the time of the call)."""
        if not 0 <= b < self.nblocks:
            raise IndexError("block %d of %d" % (b, self.nblocks))
        sz = self.mb * self.nb
        return self.data[b * sz:(b + 1) * sz].reshape((self.mb, self.nb), order="F")

    def tocsc(self):
        """The same matrix as scipy.sparse.csc_matrix (canonical order: `.data` of the result equals `.data` here)."""
        if _sp is None:     # pragma: no cover
            raise RuntimeError("BlockDiagonal.tocsc needs scipy")
        m, n = self.shape
        indptr = np.arange(n + 1, dtype=np.int64) * self.mb
        rows = (np.arange(self.nblocks, dtype=np.int64)[:, None, None] * self.mb +
                np.zeros((1, self.nb, 1), dtype=np.int64) + np.arange(self.mb, dtype=np.int64)[None, None, :]).reshape(-1)
        return _sp.csc_matrix((self.data.copy(), rows.astype(np.int32), indptr.astype(np.int32)), shape=(m, n))

    def toarray(self):
        out = np.zeros(self.shape)
        for b in range(self.nblocks):
            out[b * self.mb:(b + 1) * self.mb, b * self.nb:(b + 1) * self.nb] = self.block(b)
        return out


def _is_blockdiag(J):
    return isinstance(J, BlockDiagonal)


class BorderedBlockDiagonal:
    """J = [blkdiag(J_1 .. J_B) | C]: the Jacobian of a GLOBAL fit -- data set b has its own nb local parameters (J_b dense
    mb x nb) and ng parameters are shared by all data sets (C dense (B*mb) x ng; C_b = its rows of block b).  m = B*mb
    residuals, n = B*nb + ng parameters, the shared ones last.  The same kind of host-side container as BlockDiagonal:
    `.data` is the flat value array g_ overwrites, ordered as the nzval of `.tocsc()` -- B column-major mb x nb blocks back
    to back, then the ng border columns of m values each.
    On the device it becomes a CSC handle that knows its shape (lsq_blockdiag_bordered_create): LSMR() is the default solver,
    Cholesky() eliminates the locals block by block and factors the ng x ng Schur complement (nb + ng <= 64;
    LevenbergMarquardt only), Schur() does the same for any ng (nb <= 64), BorderedQR() solves the same damped problem by
    Householder reflectors without forming J'J (nb <= 64, any ng), QR() and BlockQR() are refused."""

    def __init__(self, nblocks, mb, nb, ng, data=None):
        nblocks, mb, nb, ng = int(nblocks), int(mb), int(nb), int(ng)
        if nblocks < 1 or mb < 1 or nb < 1 or ng < 1:
            raise DimensionMismatch(_lib.EDIM, "BorderedBlockDiagonal needs nblocks >= 1, mb >= 1, nb >= 1, ng >= 1 "
                                               "(got %d, %d, %d, %d)" % (nblocks, mb, nb, ng))
        self.nblocks, self.mb, self.nb, self.ng = nblocks, mb, nb, ng
        self.shape = (nblocks * mb, nblocks * nb + ng)
        self.nnz = nblocks * mb * (nb + ng)
        if data is None:
            self.data = np.zeros(self.nnz)
        else:
            d = np.ascontiguousarray(data, dtype=np.float64).reshape(-1)
            if d.size != self.nnz:
                raise DimensionMismatch(_lib.EDIM, "BorderedBlockDiagonal: expected %d values, got %d" % (self.nnz, d.size))
            self.data = d

    @classmethod
    def from_blocks(cls, blocks, border):
        """From a sequence of equally shaped (mb, nb) arrays and the (B*mb, ng) border."""
        blocks = [np.asarray(b, dtype=np.float64) for b in blocks]
        if not blocks or blocks[0].ndim != 2:
            raise DimensionMismatch(_lib.EDIM, "BorderedBlockDiagonal.from_blocks needs a non-empty sequence of matrices")
        mb, nb = blocks[0].shape
        for k, b in enumerate(blocks):
            if b.shape != (mb, nb):
                raise DimensionMismatch(_lib.EDIM, "BorderedBlockDiagonal.from_blocks: block %d is %s, block 0 is %s"
                                        % (k, b.shape, (mb, nb)))
        border = np.asarray(border, dtype=np.float64)
        if border.ndim != 2 or border.shape[0] != len(blocks) * mb or border.shape[1] < 1:
            raise DimensionMismatch(_lib.EDIM, "BorderedBlockDiagonal.from_blocks: the border is %s, expected (%d, ng >= 1)"
                                    % (border.shape, len(blocks) * mb))
        out = cls(len(blocks), mb, nb, border.shape[1])
        for k, b in enumerate(blocks):
            out.block(k)[:, :] = b
        out.border[:, :] = border
        return out

    def block(self, b):
        """Block b as an (mb, nb) VIEW into `.data` (as it is bound at the time of the call)."""
        if not 0 <= b < self.nblocks:
            raise IndexError("block %d of %d" % (b, self.nblocks))
        sz = self.mb * self.nb
        return self.data[b * sz:(b + 1) * sz].reshape((self.mb, self.nb), order="F")

    @property
    def border(self):
        """The shared columns as an (m, ng) column-major VIEW into `.data`."""
        return self.data[self.nblocks * self.mb * self.nb:].reshape((self.shape[0], self.ng), order="F")

    def border_block(self, b):
        """C_b: rows b*mb .. of the border, an (mb, ng) VIEW into `.data`."""
        if not 0 <= b < self.nblocks:
            raise IndexError("block %d of %d" % (b, self.nblocks))
        return self.border[b * self.mb:(b + 1) * self.mb, :]

    def tocsc(self):
        """The same matrix as scipy.sparse.csc_matrix (canonical order: `.data` of the result equals `.data` here)."""
        if _sp is None:     # pragma: no cover
            raise RuntimeError("BorderedBlockDiagonal.tocsc needs scipy")
        m, n = self.shape
        nloc = self.nblocks * self.nb
        indptr = np.concatenate([np.arange(nloc + 1, dtype=np.int64) * self.mb,
                                 nloc * self.mb + np.arange(1, self.ng + 1, dtype=np.int64) * m])
        rows = (np.arange(self.nblocks, dtype=np.int64)[:, None, None] * self.mb +
                np.zeros((1, self.nb, 1), dtype=np.int64) + np.arange(self.mb, dtype=np.int64)[None, None, :]).reshape(-1)
        rows = np.concatenate([rows, np.tile(np.arange(m, dtype=np.int64), self.ng)])
        return _sp.csc_matrix((self.data.copy(), rows.astype(np.int32), indptr.astype(np.int32)), shape=(m, n))

    def toarray(self):
        out = np.zeros(self.shape)
        for b in range(self.nblocks):
            out[b * self.mb:(b + 1) * self.mb, b * self.nb:(b + 1) * self.nb] = self.block(b)
        out[:, self.nblocks * self.nb:] = self.border
        return out


BORDERED_DOGLEG_TEXT = ("Dogleg(Cholesky()) is not available on a bordered block-diagonal Jacobian: the reference's pivoted "
                        "factorisation orders local and shared columns together, which does not split into blocks. "
                        "Use LevenbergMarquardt(Cholesky()) or LSMR()")


SCHUR_HANDLE_TEXT = ("Schur() needs a BorderedBlockDiagonal Jacobian (got a %s of shape %s). Use Cholesky() or QR() on a dense "
                     "Jacobian, Cholesky() or BlockQR() on a BlockDiagonal one, LSMR() on a sparse one")
SCHUR_NB_TEXT = "Schur() on a BorderedBlockDiagonal Jacobian needs nb <= 64 (got nb = %d, ng = %d). Use LSMR()"
BORDERED_QR_HANDLE_TEXT = ("BorderedQR() needs a BorderedBlockDiagonal Jacobian (got a %s of shape %s). Use QR() on a dense "
                           "Jacobian, BlockQR() on a BlockDiagonal one, LSMR() on a sparse one")
BORDERED_QR_NB_TEXT = "BorderedQR() on a BorderedBlockDiagonal Jacobian needs nb <= 64 (got nb = %d, ng = %d). Use LSMR()"


def _is_bordered(J):
    return isinstance(J, BorderedBlockDiagonal)



def default_solver(solver, J):
    """types.jl:114-121"""
    matrix_free = type(J).__name__ == "DeviceOperator"
    if solver is None:
        return LSMR() if (_is_sparse(J) or _is_blockdiag(J) or _is_bordered(J) or matrix_free) else QR()
    if matrix_free and not isinstance(solver, LSMR):
        raise ArgumentError(_lib.EARG, "a matrix-free Jacobian works with LSMR() only (README.md:37-47)")
    if isinstance(solver, Schur):
        if not _is_bordered(J):
            raise ArgumentError(_lib.EARG, SCHUR_HANDLE_TEXT % (type(J).__name__, tuple(getattr(J, "shape", ()))))
        if J.nb > 64:
            raise ArgumentError(_lib.EARG, SCHUR_NB_TEXT % (J.nb, J.ng))
        return solver
    if isinstance(solver, BorderedQR):
        if not _is_bordered(J):
            raise ArgumentError(_lib.EARG, BORDERED_QR_HANDLE_TEXT % (type(J).__name__, tuple(getattr(J, "shape", ()))))
        if J.nb > 64:
            raise ArgumentError(_lib.EARG, BORDERED_QR_NB_TEXT % (J.nb, J.ng))
        return solver
    if _is_bordered(J):
        if isinstance(solver, QR):
            raise ArgumentError(_lib.EARG, "solver QR() is not available for a BorderedBlockDiagonal Jacobian. "
                                           "Choose between Cholesky() and LSMR()")
        if isinstance(solver, BlockQR):
            raise ArgumentError(_lib.EARG, "BlockQR() is not available for a BorderedBlockDiagonal Jacobian: the shared columns "
                                           "couple the blocks. Choose between Cholesky() and LSMR()")
        if isinstance(solver, Cholesky) and J.nb + J.ng > 64:
            raise ArgumentError(_lib.EARG, "Cholesky() on a BorderedBlockDiagonal Jacobian needs nb + ng <= 64 "
                                           "(got nb = %d, ng = %d). Use LSMR()" % (J.nb, J.ng))
        return solver
    if isinstance(solver, QR) and (_is_sparse(J) or _is_blockdiag(J)):
        raise ArgumentError(_lib.EARG, "solver QR() is not available for sparse Jacobians. "
                                       "Choose between Cholesky() and LSMR()")
    if isinstance(solver, BlockQR):
        if not _is_blockdiag(J):
            raise ArgumentError(_lib.EARG, "BlockQR() needs a BlockDiagonal Jacobian with blocks of at most 64 columns "
                                           "(got a %s of shape %s). Use QR() on a dense Jacobian, LSMR() on a sparse one"
                                           % (type(J).__name__, tuple(getattr(J, "shape", ()))))
        if J.nb > 64:
            raise ArgumentError(_lib.EARG, "BlockQR() needs blocks of at most 64 columns (got %d blocks of %d x %d). "
                                           "Use LSMR()" % (J.nblocks, J.mb, J.nb))
    return solver


def default_optimizer(optimizer, solver, J=None):
    """types.jl:123-127.  On a BorderedBlockDiagonal J, Cholesky(), Schur() and BorderedQR() come with LevenbergMarquardt
    (Dogleg with any of them does not exist there and is refused)."""
    if isinstance(solver, (Schur, BorderedQR)) or (_is_bordered(J) and isinstance(solver, Cholesky)):
        if isinstance(optimizer, Dogleg):
            raise ArgumentError(_lib.EARG, BORDERED_DOGLEG_TEXT)
        return LevenbergMarquardt(solver)
    if isinstance(optimizer, Dogleg):
        return Dogleg(solver)
    if isinstance(optimizer, LevenbergMarquardt):
        return LevenbergMarquardt(solver)
    if isinstance(solver, LSMR):
        return LevenbergMarquardt(solver)
    return Dogleg(solver)


# ------------------------------------------------------------------------------------------------
# device context and buffers
# ------------------------------------------------------------------------------------------------
class Context:
    """One per device/stream (SURVEY 8b 'Threading'); fails loudly without a HIP device."""

    def __init__(self, device=0, stream=None):
        h = C.c_void_p()
        check(lib().lsq_ctx_create(int(device), stream, C.byref(h)))
        self.h = h
        self.device = device

    def sync(self):
        check(lib().lsq_ctx_sync(self.h))

    def device_info(self):
        """lsq_ctx_device_info: {'num_cus', 'num_xcds', 'arch'} -- what the launch heuristics see (256 CUs unpartitioned)."""
        a, b = C.c_int(0), C.c_int(0)
        name = C.create_string_buffer(128)
        check(lib().lsq_ctx_device_info(self.h, C.byref(a), C.byref(b), name, 128))
        return {"num_cus": a.value, "num_xcds": b.value, "arch": name.value.decode()}

    @property
    def num_cus(self):
        return self.device_info()["num_cus"]

    def fallback_stats(self):
        """lsq_ctx_fallback_stats: how often the co-residency fast paths of this context's solvers gave up on a bounded wait."""
        g = (C.c_int * 4)()
        check(lib().lsq_ctx_fallback_stats(self.h, g))
        return dict(zip(("chol_one_launch", "tri_pipeline", "qr_exchange", "cholqr_panel"), (int(v) for v in g)))

    def tail_stats(self):
        """lsq_ctx_tail_stats: (LSMR solves whose follow-up kernels were queued behind a guessed last iteration, wrong guesses)."""
        v = (C.c_longlong * 2)()
        check(lib().lsq_ctx_tail_stats(self.h, v))
        return int(v[0]), int(v[1])

    def commit_step_stats(self):
        """lsq_ctx_commit_step_stats: k_lsmr_commit_step launches that (found their solve over and took the LM step, found it
        unfinished)."""
        v = (C.c_longlong * 2)()
        check(lib().lsq_ctx_commit_step_stats(self.h, v))
        return int(v[0]), int(v[1])

    def occupy(self, workgroups, lds_bytes=65536, milliseconds=10.0):
        """A neighbour on the device (lsq_bench_occupy): workgroups that hold LDS and spin, on a stream of their own."""
        check(lib().lsq_bench_occupy(self.h, int(workgroups), int(lds_bytes), float(milliseconds)))

    def occupy_wait(self):
        check(lib().lsq_bench_occupy_wait(self.h))

    def close(self):
        if self.h:
            lib().lsq_ctx_destroy(self.h)
            self.h = None


_DEFAULT_CTX = {}


def default_context(device=0):
    if device not in _DEFAULT_CTX:
        _DEFAULT_CTX[device] = Context(device)
    return _DEFAULT_CTX[device]


class DeviceVector:
    """fp64 vector in HBM (the `HipVector` of SURVEY 8b)."""

    def __init__(self, ctx, n, data=None):
        self.ctx, self.n = ctx, int(n)
        p = C.c_void_p()
        check(lib().lsq_malloc(ctx.h, max(self.n, 1) * 8, C.byref(p)))
        self.ptr = p
        if data is not None:
            self.set(data)
        else:
            check(lib().lsq_fill(ctx.h, self.n, 0.0, self.ptr))

    @classmethod
    def borrow(cls, ctx, n, ptr):
        """A view of device memory owned by someone else (never freed here)."""
        v = cls.__new__(cls)
        v.ctx, v.n, v.ptr, v._borrowed = ctx, int(n), ptr, True
        return v

    def set(self, data):
        a = np.ascontiguousarray(data, dtype=np.float64)
        if a.size != self.n:
            raise DimensionMismatch(_lib.EDIM, "vector has length %d, expected %d" % (a.size, self.n))
        check(lib().lsq_h2d(self.ctx.h, self.ptr, a.ctypes.data_as(C.c_void_p), self.n * 8))

    def get(self):
        out = np.empty(self.n)
        check(lib().lsq_d2h(self.ctx.h, out.ctypes.data_as(C.c_void_p), self.ptr, self.n * 8))
        return out

    def free(self):
        if self.ptr and not getattr(self, "_borrowed", False):
            lib().lsq_free(self.ctx.h, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _ptr(v):
    return None if v is None else v.ptr


class PinnedBuffer:
    """Page-locked host memory (lsq_host_alloc) as a float64 numpy array: what a host-side g! should write the Jacobian
    values into, so that the upload after every g!(J, x) runs asynchronously at the PCIe rate
    (DeviceMatrix.set_values_async).  `array` is only valid until free()."""

    def __init__(self, ctx, n):
        self.ctx, self.n = ctx, int(n)
        p = C.c_void_p()
        check(lib().lsq_host_alloc(ctx.h, max(self.n, 1) * 8, C.byref(p)))
        self.ptr = p
        self.array = np.ctypeslib.as_array(C.cast(p, _lib.c_dp), shape=(max(self.n, 1),))[:self.n]

    def free(self):
        if self.ptr:
            self.array = None
            lib().lsq_host_free(self.ctx.h, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def mat_layout(h):
    """lsq_mat_layout of a raw handle as a dict (DeviceMatrix.layout(); a TanhProblem's `.J` takes it too)."""
    o = (C.c_int * 12)()
    check(lib().lsq_mat_layout(h, o))
    plan = {-1: None, 0: "stream", 1: "wave", 2: "block"}
    return dict(kind={0: "dense", 1: "csc", 2: "operator"}[o[0]],
                srows=dict(active=bool(o[1]), ncw=o[2], wrows=o[3]),
                scols=dict(active=bool(o[4]), ngw=o[5], ncb=o[6]),
                nwin=o[7], csr_plan=plan[o[8]], csc_plan=plan[o[9]],
                colscale={0: None, 1: "fused", 2: "materialising"}[o[10]], csc_fresh=bool(o[11]))


class DeviceMatrix:
    """Jacobian handle: dense column-major or CSC (+ CSR mirror) -- `HipDense` / `HipCSC`."""

    def __init__(self, ctx, J):
        self.ctx = ctx
        h = C.c_void_p()
        L = lib()
        self.blockdiag = None
        self.bordered = None
        if _is_bordered(J):
            self.sparse = True          # (values are addressed like a CSC handle's nzval)
            self.bordered = (J.nblocks, J.mb, J.nb, J.ng)
            self.m, self.n = J.shape
            check(L.lsq_blockdiag_bordered_create(ctx.h, J.nblocks, J.mb, J.nb, J.ng, C.byref(h)))
            self.h = h
            self.nnz = J.nnz
            self.set_values(J.data)
        elif _is_blockdiag(J):
            self.sparse = True          # (values are addressed like a CSC handle's nzval)
            self.blockdiag = (J.nblocks, J.mb, J.nb)
            self.m, self.n = J.shape
            check(L.lsq_blockdiag_create(ctx.h, J.nblocks, J.mb, J.nb, C.byref(h)))
            self.h = h
            self.nnz = J.nnz
            self.set_values(J.data)
        elif _is_sparse(J):
            S = J.tocsc()
            S.sort_indices()
            self.sparse = True
            self.m, self.n = S.shape
            self.colptr = np.ascontiguousarray(S.indptr, dtype=np.int32)
            self.rowval = np.ascontiguousarray(S.indices, dtype=np.int32)
            check(L.lsq_csc_create(ctx.h, self.m, self.n, self.colptr.ctypes.data_as(_lib.c_ip),
                                   self.rowval.ctypes.data_as(_lib.c_ip), C.byref(h)))
            self.h = h
            self.nnz = int(S.nnz)
            self.set_values(S.data)
        else:
            A = np.asarray(J, dtype=np.float64)
            if A.ndim != 2:
                raise DimensionMismatch(_lib.EDIM, "J must be a matrix")
            self.sparse = False
            self.m, self.n = A.shape
            check(L.lsq_dense_create(ctx.h, self.m, self.n, C.byref(h)))
            self.h = h
            self.nnz = self.m * self.n
            self.set_values(np.asfortranarray(A).reshape(-1, order="F"))

    def set_values(self, vals):
        v = np.ascontiguousarray(vals, dtype=np.float64)
        if v.size != self.nnz:
            raise DimensionMismatch(_lib.EDIM, "expected %d values, got %d" % (self.nnz, v.size))
        check(lib().lsq_mat_set_values(self.h, v.ctypes.data_as(_lib.c_dp)))

    def set_values_async(self, pinned):
        """Upload from a PinnedBuffer without blocking the host (lsq_mat_set_values_async): later uses of J wait for the
        copy on the device; the buffer must not be rewritten before upload_wait() (or a call that reads results back)."""
        if pinned.n != self.nnz:
            raise DimensionMismatch(_lib.EDIM, "expected %d values, got %d" % (self.nnz, pinned.n))
        check(lib().lsq_mat_set_values_async(self.h, C.cast(pinned.ptr, _lib.c_dp)))

    def upload_wait(self):
        check(lib().lsq_mat_upload_wait(self.h))

    def values(self):
        out = np.empty(self.nnz)
        check(lib().lsq_mat_get_values(self.h, out.ctypes.data_as(_lib.c_dp)))
        return out

    def refresh(self):
        """lsq_mat_refresh: after a device-side write through lsq_mat_values."""
        check(lib().lsq_mat_refresh(self.h))

    def scale_rows(self, w):
        """lsq_mat_scale_rows: J <- diag(w) J, every stored entry times the factor of its row (one product), in every layout
        of the handle.  `w`: a DeviceVector of m factors or m host values.  An operator or a column-scaled handle raises
        ArgumentError."""
        dw = w if hasattr(w, "ptr") else DeviceVector(self.ctx, self.m, w)
        if dw.n != self.m:
            raise DimensionMismatch(_lib.EDIM, "row factors have length %d, expected %d" % (dw.n, self.m))
        check(lib().lsq_mat_scale_rows(self.h, dw.ptr))

    def layout(self):
        """lsq_mat_layout: which layouts the handle built and which mode it is in (host code, changes nothing)."""
        return mat_layout(self.h)

    def blockdiag_info(self):
        """lsq_mat_blockdiag_info: (nblocks, mb, nb); (0, 0, 0) for a handle that is not block-diagonal."""
        a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
        check(lib().lsq_mat_blockdiag_info(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def bordered_info(self):
        """lsq_mat_bordered_info: (nblocks, mb, nb, ng); (0, 0, 0, 0) for a handle that is not bordered block-diagonal."""
        a, b, c, d = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        check(lib().lsq_mat_bordered_info(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return a.value, b.value, c.value, d.value

    def set_colscale(self, s):
        """J = V diag(s) (lsq_mat_set_colscale): the values held now are V, `s` a DeviceVector of n factors that stays alive
        (and may be rewritten, followed by colscale_changed()) as long as the scale is set; None removes it."""
        if s is not None and s.n != self.n:
            raise DimensionMismatch(_lib.EDIM, "column scale has length %d, expected %d" % (s.n, self.n))
        check(lib().lsq_mat_set_colscale(self.h, s.ptr if s is not None else None))
        self._colscale = s

    def colscale_changed(self):
        check(lib().lsq_mat_colscale_changed(self.h))

    def set_fd_colouring(self, colours=None):
        """lsq_mat_set_fd_colouring: attach a column colouring to a plain CSC handle, after which fd_jacobian_ and the loops
        with a NULL g! take central differences on it.  None: the greedy colouring of the handle's own pattern; else n colours
        0 .. ncolours-1 (validated by the library: ArgumentError).  Returns the number of colours; a second call replaces
        the first."""
        ptr = None
        if colours is not None:
            a = np.ascontiguousarray(colours, dtype=np.int32)
            if a.ndim != 1 or a.size != self.n:
                raise ArgumentError(_lib.EARG, "a colouring has one colour per column: expected %d, got %d" % (self.n, a.size))
            ptr = a.ctypes.data_as(_lib.c_ip)
        nc = C.c_int(0)
        check(lib().lsq_mat_set_fd_colouring(self.h, ptr, C.byref(nc)))
        return nc.value

    def fd_colouring(self):
        """lsq_mat_fd_colouring: (int32 array of n colours, ncolours); (None, 0) when no colouring is attached."""
        nc = C.c_int(0)
        check(lib().lsq_mat_fd_colouring(self.h, None, C.byref(nc)))
        if nc.value == 0:
            return None, 0
        out = np.zeros(self.n, dtype=np.int32)
        check(lib().lsq_mat_fd_colouring(self.h, out.ctypes.data_as(_lib.c_ip), C.byref(nc)))
        return out, nc.value

    def free(self):
        if self.h:
            lib().lsq_mat_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# --- operator interface (README.md:37-47) on device objects -------------------------------------
def mul_(y, J, x, alpha=1.0, beta=0.0, trans=False):
    """mul!(y, J, x, alpha, beta) / mul!(y, J', x, alpha, beta)"""
    check(lib().lsq_mul(J.h, 1 if trans else 0, float(alpha), x.ptr, float(beta), y.ptr))
    return y


def colsumabs2_(out, J):
    check(lib().lsq_colsumabs2(J.h, out.ptr))
    return out


def rowsumabs2_(out, J):
    """rowsumabs2!(out, J) (utils.jl:153-161): what colsumabs2! of an adjoint Jacobian computes."""
    check(lib().lsq_rowsumabs2(J.h, out.ptr))
    return out


# BLAS-1 on device vectors -- exactly what lsmr.jl:30-44 and the optimizer loops ask of a vector type
def axpy_(a, x, y):
    """axpy!(a, x, y): y += a*x"""
    check(lib().lsq_axpy(x.ctx.h, x.n, float(a), x.ptr, y.ptr))
    return y


def rmul_(x, a):
    """rmul!(x, a)"""
    check(lib().lsq_scal(x.ctx.h, x.n, float(a), x.ptr))
    return x


def copyto_(dst, src):
    """copyto!(dst, src)"""
    check(lib().lsq_copy(src.ctx.h, src.n, src.ptr, dst.ptr))
    return dst


def fill_(x, a):
    """fill!(x, a)"""
    check(lib().lsq_fill(x.ctx.h, x.n, float(a), x.ptr))
    return x


def clamp_(x, lo, hi):
    """clamp!(x, lo, hi)"""
    check(lib().lsq_clamp(x.ctx.h, x.n, float(lo), float(hi), x.ptr))
    return x


def ediv_(out, x, y):
    """map!(/, out, x, y)"""
    check(lib().lsq_ediv(x.ctx.h, x.n, x.ptr, y.ptr, out.ptr))
    return out


def box_clip_(dx, x, lower=None, upper=None):
    """the step clipping of levenberg_marquardt.jl:89-98 / dogleg.jl:148-160"""
    check(lib().lsq_box_clip(x.ctx.h, x.n, dx.ptr, x.ptr, _ptr(lower), _ptr(upper)))
    return dx


def vsum(x):
    return _scalar(lib().lsq_sum, x.ctx, x.n, x.ptr)


def first_nonfinite(x):
    """check_isfinite (utils.jl:70-75): first non-finite index or -1"""
    r = C.c_int(0)
    check(lib().lsq_first_nonfinite(x.ctx.h, x.n, x.ptr, C.byref(r)))
    return r.value


def _scalar(fn, ctx, n, *ptrs):
    r = C.c_double(0.0)
    check(fn(ctx.h, n, *ptrs, C.byref(r)))
    return r.value


def sumsq(x):
    return _scalar(lib().lsq_sumsq, x.ctx, x.n, x.ptr)


def norm(x):
    return _scalar(lib().lsq_nrm2, x.ctx, x.n, x.ptr)


def wdot(x, y, w):
    return _scalar(lib().lsq_wdot, x.ctx, x.n, x.ptr, y.ptr, w.ptr)


def wnorm(x, w):
    return float(np.sqrt(wdot(x, x, w)))


def maxabs(x):
    return _scalar(lib().lsq_amax, x.ctx, x.n, x.ptr)


def maxabs_projected_gradient(g, x, lower=None, upper=None):
    return _scalar(lib().lsq_amax_projected, g.ctx, g.n, g.ptr, x.ptr, _ptr(lower), _ptr(upper))


def set_exact(on=None):
    """Reference-order arithmetic for small problems (include/lsqhip.h: lsq_set_exact).
    True / False force it on / off; None restores the default (on unless LSQ_EXACT=0)."""
    check(lib().lsq_set_exact(-1 if on is None else (1 if on else 0)))


def debug_set(launch_jitter_us=None, serial=None):
    """Process-wide debug modes of the library (include/lsqhip.h: lsq_debug_set): random host stalls in front of the
    kernel launches / serialised launches (1: same kernels, bit-identical results; 2: also without the in-kernel
    workgroup exchanges).  None leaves a setting alone."""
    check(lib().lsq_debug_set(-1 if launch_jitter_us is None else int(launch_jitter_us), -1 if serial is None else int(serial)))


def debug_get():
    """(launch_jitter_us, serial, stalls injected so far)"""
    import ctypes as _C
    a, b, c = _C.c_int(0), _C.c_int(0), _C.c_longlong(0)
    check(lib().lsq_debug_get(_C.byref(a), _C.byref(b), _C.byref(c)))
    return a.value, b.value, c.value


class DeviceOperator:
    """A matrix-free Jacobian (README.md:37-47 of the reference: any type with mul!, the adjoint's mul!,
    colsumabs2!, size and eltype works with LSMR).  `mul(trans, x, out)` writes J*x (trans = False, m
    entries) or J'*x (trans = True, n entries) into the DeviceVector `out`; `colsumabs2(out)` the n column
    sums of squares.  Both are called on the host with device vectors; use `refresh()` after the operator
    changed (what g! does for a stored Jacobian).  LSMR only."""
    sparse = True   # (types.jl:114-121: a non-dense Jacobian defaults to LSMR)

    def __init__(self, ctx, m, n, mul, colsumabs2):
        self.ctx, self.m, self.n = ctx, int(m), int(n)
        self.shape = (self.m, self.n)
        self._errors = []

        def _mul(trans, d_x, d_out, _user):
            try:
                t = bool(trans)
                mul(t, DeviceVector.borrow(ctx, self.m if t else self.n, d_x),
                    DeviceVector.borrow(ctx, self.n if t else self.m, d_out))
                ctx.sync()
                return 0
            except Exception as e:
                self._errors.append(e)
                return 1

        def _cs(d_out, _user):
            try:
                colsumabs2(DeviceVector.borrow(ctx, self.n, d_out))
                ctx.sync()
                return 0
            except Exception as e:
                self._errors.append(e)
                return 1

        self._cbs = (_lib.OP_MUL_CALLBACK(_mul), _lib.OP_COLSUM_CALLBACK(_cs))
        h = C.c_void_p()
        check(lib().lsq_op_create(ctx.h, self.m, self.n, self._cbs[0], self._cbs[1], None, C.byref(h)))
        self.h = h

    def refresh(self):
        check(lib().lsq_mat_refresh(self.h))

    def free(self):
        if self.h:
            lib().lsq_mat_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class AllocatedSolver:
    """AbstractAllocatedSolver(nls, optimizer) + ldiv! (the L2 plug point)."""

    def __init__(self, J, solver, for_lm):
        h = C.c_void_p()
        check(lib().lsq_solver_create(J.ctx.h, J.h, solver.kind, 1 if for_lm else 0, C.byref(h)))
        self.h, self.J, self.kind = h, J, solver.kind
        self._pc = None
        if getattr(solver, "P", None) is not None:
            self._pc = _general_precond_trampolines(solver, J.ctx, J)
            check(lib().lsq_solver_set_general_preconditioner(self.h, self._pc[0], self._pc[1], None))
        elif getattr(solver, "preconditioner", None) is not None:
            self._pc = _precond_trampoline(solver.preconditioner, J.ctx, J)
            check(lib().lsq_solver_set_preconditioner(self.h, self._pc, None))

    def set_row_allreduce(self, hook, global_rows):
        """lsq_solver_set_row_allreduce: J (and y) of the coming ldiv! calls are this rank's ROW BLOCK of one problem with
        `global_rows` residuals; `hook` (rowshard.RcclRowAllreduce / HostStagedRowAllreduce, or None to switch it off) sums
        the replicated n-vectors over the ranks.  LSMR() only."""
        self._row_hook = hook       # (keeps the ctypes callback alive)
        if hook is None:
            check(lib().lsq_solver_set_row_allreduce(self.h, _lib.ROW_ALLREDUCE_CALLBACK(), None, 0))
        else:
            check(lib().lsq_solver_set_row_allreduce(self.h, hook.callback, hook.user, int(global_rows)))

    def ldiv_(self, x, y, damp=None):
        """ldiv!(x, J, y[, damp], A) -> (x, nmul)"""
        n = C.c_int(0)
        if damp is None:
            check(lib().lsq_ldiv(self.h, self.J.h, y.ptr, x.ptr, C.byref(n)))
        else:
            check(lib().lsq_ldiv_damped(self.h, self.J.h, y.ptr, damp.ptr, x.ptr, C.byref(n)))
        return x, n.value

    def info(self):
        it, st, rk = C.c_int(0), C.c_int(0), C.c_int(0)
        check(lib().lsq_solver_info(self.h, C.byref(it), C.byref(st), C.byref(rk)))
        path = C.c_int(0)
        check(lib().lsq_solver_qr_path(self.h, C.byref(path)))
        cpath = C.c_int(0)
        check(lib().lsq_solver_chol_path(self.h, C.byref(cpath)))
        lpath = C.c_int(0)
        check(lib().lsq_solver_lsmr_path(self.h, C.byref(lpath)))
        panel = C.c_int(0)
        check(lib().lsq_solver_qr_panel(self.h, C.byref(panel)))
        bpath, bblock = C.c_int(0), C.c_int(-1)
        check(lib().lsq_solver_blockdiag_path(self.h, C.byref(bpath), C.byref(bblock)))
        block_ranks = None
        if self.kind == _lib.BLOCK_QR:
            block_ranks = np.zeros(self.J.blockdiag_info()[0], dtype=np.int32)
            check(lib().lsq_solver_blockdiag_ranks(self.h, block_ranks.ctypes.data_as(_lib.c_ip)))
        return dict(blockdiag_path={0: None, 1: "batched-unpivoted", 2: "batched-pivoted", 3: "batched-qr",
                                    4: "bordered-schur", 5: "bordered-schur-tiled", 6: "bordered-qr"}[bpath.value],
                    blockdiag_block=bblock.value, block_ranks=block_ranks,
                    lsmr_iter=it.value, lsmr_istop=st.value, qr_rank=rk.value,
                    lsmr_path={0: None, 1: "reference-order", 2: "four-launch", 3: "three-launch", 4: "general"}[lpath.value],
                    qr_panel={0: None, 1: "householder-steps", 2: "cholqr2"}[panel.value],
                    qr_path={0: None, 1: "one-stage", 2: "two-stage-pivoted", 3: "two-stage-certified"}[path.value],
                    chol_path={0: None, 1: "one-workgroup", 2: "blocked", 3: "blocked-certified", 4: "blocked-one-launch"}[cpath.value])

    def covariance(self, f=None, stderr=True):
        """lsq_solver_covariance at the values J holds now: a Covariance.  `f`: None (the unscaled inv(J'J)), or the residual
        there (DeviceVector or m host values) -- per-block variances on a block-diagonal handle, one on a bordered handle."""
        J = self.J
        if J.bordered is not None:
            B, _, nb, ng = J.bordered
        elif J.blockdiag is not None:
            (B, _, nb), ng = J.blockdiag, 0
        else:
            B, nb, ng = 0, 0, 0            # (refused by the library, with its message)
        df = f if (f is None or hasattr(f, "ptr")) else DeviceVector(J.ctx, J.m, f)
        dcov = DeviceVector(J.ctx, B * nb * nb + ng * ng)
        dse = DeviceVector(J.ctx, J.n) if stderr else None
        info = np.zeros(max(B, 1), dtype=np.int32)
        check(lib().lsq_solver_covariance(self.h, J.h, _ptr(df), dcov.ptr, _ptr(dse), info.ctypes.data_as(_lib.c_ip)))
        return Covariance(B, nb, ng, dcov.get(), dse.get() if stderr else None, info[:B] if not ng else None)

    def dense_covariance(self, f=None, stderr=True):
        """lsq_dense_covariance at the values the dense J holds now: a DenseCovariance.  `f`: None (the unscaled inv(J'J)), or
        the residual there (DeviceVector or m host values): s^2 = sum(f.^2) / (m - n)."""
        J = self.J
        df = f if (f is None or hasattr(f, "ptr")) else DeviceVector(J.ctx, J.m, f)
        n = J.n if not J.sparse else 0       # (any other handle is refused by the library, with its message)
        dcov = DeviceVector(J.ctx, n * n)
        dse = DeviceVector(J.ctx, J.n) if stderr else None
        info = np.zeros(1, dtype=np.int32)
        check(lib().lsq_dense_covariance(self.h, J.h, _ptr(df), dcov.ptr, _ptr(dse), info.ctypes.data_as(_lib.c_ip)))
        return DenseCovariance(J.n, dcov.get(), dse.get() if stderr else None)

    def dense_qr_covariance(self, f=None, stderr=True):
        """lsq_dense_qr_covariance at the values the dense J holds now, from the QR() factor of this solver (J'J is not formed):
        a DenseCovariance.  `f` as for dense_covariance.  A rank-deficient J raises RankDeficientException."""
        J = self.J
        df = f if (f is None or hasattr(f, "ptr")) else DeviceVector(J.ctx, J.m, f)
        n = J.n if not J.sparse else 0       # (any other handle is refused by the library, with its message)
        dcov = DeviceVector(J.ctx, n * n)
        dse = DeviceVector(J.ctx, J.n) if stderr else None
        info = np.zeros(1, dtype=np.int32)
        check(lib().lsq_dense_qr_covariance(self.h, J.h, _ptr(df), dcov.ptr, _ptr(dse), info.ctypes.data_as(_lib.c_ip)))
        return DenseCovariance(J.n, dcov.get(), dse.get() if stderr else None)

    def sparse_covariance(self, f=None, cov=True, stderr=True):
        """lsq_sparse_covariance at the values the sparse (CSC) J holds now, on this LSMR() solver: a DenseCovariance with
        `.chol_path`, the factorisation that ran on J'J.  `f` as for dense_covariance.  cov=False: the standard errors only --
        no n x n output is allocated anywhere; `.cov` is then None."""
        J = self.J
        df = f if (f is None or hasattr(f, "ptr")) else DeviceVector(J.ctx, J.m, f)
        n = J.n if (J.sparse and cov) else 0   # (any other handle is refused by the library, with its message)
        dcov = DeviceVector(J.ctx, n * n) if cov else None
        dse = DeviceVector(J.ctx, J.n) if stderr else None
        info = np.zeros(1, dtype=np.int32)
        check(lib().lsq_sparse_covariance(self.h, J.h, _ptr(df), _ptr(dcov), _ptr(dse), info.ctypes.data_as(_lib.c_ip)))
        return DenseCovariance(J.n, dcov.get() if cov else None, dse.get() if stderr else None,
                               chol_path=self.info()["chol_path"])

    def bordered_qr_covariance(self, f=None, cov=True, stderr=True, cross=False):
        """lsq_bordered_qr_covariance at the values the bordered J holds now, from the factor of this BorderedQR() solver (J'J is
        not formed): a BorderedCovariance.  `f`: None (the unscaled inv(J'J)), or the residual (DeviceVector or m host values):
        one variance s^2 = sum(f.^2) / (m - n).  cross=True: the (B nb) x ng local-shared cross-covariances as well.  A zero or
        non-finite local column, or a rank-deficient border, raises RankDeficientException."""
        J = self.J
        B, _, nb, ng = J.bordered if J.bordered is not None else (0, 0, 0, 0)   # (any other handle is refused by the library)
        df = f if (f is None or hasattr(f, "ptr")) else DeviceVector(J.ctx, J.m, f)
        dcov = DeviceVector(J.ctx, B * nb * nb + ng * ng) if cov else None
        dse = DeviceVector(J.ctx, J.n) if stderr else None
        dcr = DeviceVector(J.ctx, B * nb * ng) if cross else None
        info = np.zeros(2, dtype=np.int32)
        check(lib().lsq_bordered_qr_covariance(self.h, J.h, _ptr(df), _ptr(dcov), _ptr(dse), _ptr(dcr),
                                               info.ctypes.data_as(_lib.c_ip)))
        return BorderedCovariance(B, nb, ng, dcov.get() if cov else None, dse.get() if stderr else None,
                                  dcr.get() if cross else None, rank=int(info[1]))

    def dense_qr_leverage(self, f=None, A=None):
        """lsq_dense_qr_leverage at the values the dense J holds now, from the QR() factor of this solver: a Leverage.
        A=None: the rows of J, `.q` = `.h` the m leverages; with the residual `f` (DeviceVector or m host values) also `.se`,
        `.studentized`, `.cook` and `.s2`.  A: p new rows (a p x n array, or n values for one row) in the parameter space the
        handle means: `.q` the p quadratic forms a' inv(J'J) a and, with `f`, `.se` = sqrt(s2 q), the standard error of the
        prediction: the confidence band is y^ +- t * se.  A rank-deficient J raises RankDeficientException."""
        J = self.J
        dense = not getattr(J, "sparse", True)
        m, n = (J.m, J.n) if dense else (0, 0)      # (any other handle is refused by the library, with its message)
        df = f if (f is None or hasattr(f, "ptr")) else DeviceVector(J.ctx, J.m, f)
        dA, p = None, 0
        if A is not None:
            A = np.asarray(A, dtype=np.float64)
            A = A.reshape((1, -1)) if A.ndim == 1 else A
            if A.ndim != 2 or A.shape[1] != J.n:
                raise DimensionMismatch(_lib.EDIM, "A has shape %s, expected (p, %d)" % (A.shape, J.n))
            p = A.shape[0]
            dA = DeviceVector(J.ctx, A.size, np.asfortranarray(A).reshape(-1, order="F"))
        rows = p if A is not None else m
        own = A is None and f is not None
        dq = DeviceVector(J.ctx, rows)
        dse = DeviceVector(J.ctx, rows) if f is not None else None
        dt = DeviceVector(J.ctx, rows) if own else None
        dck = DeviceVector(J.ctx, rows) if own else None
        s2, info = C.c_double(0.0), np.zeros(1, dtype=np.int32)
        check(lib().lsq_dense_qr_leverage(self.h, J.h, _ptr(dA), p, p, _ptr(df), dq.ptr, _ptr(dse), _ptr(dt), _ptr(dck),
                                          C.byref(s2) if f is not None else None, info.ctypes.data_as(_lib.c_ip)))
        return Leverage(dq.get(), se=None if dse is None else dse.get(), studentized=None if dt is None else dt.get(),
                        cook=None if dck is None else dck.get(), s2=s2.value if f is not None else None, rank=int(info[0]))

    def leverage(self, f=None):
        """lsq_solver_leverage at the values the block-diagonal J holds now, on this Cholesky() solver: a Leverage over all
        B * mb rows with `.block(b)`; `.s2` the B per-block variances and `.info` per block 0 or the column at which its
        factorisation failed (that block is NaN).  `f`: None (the leverages alone) or the residual."""
        J = self.J
        B, mb, _ = J.blockdiag if getattr(J, "blockdiag", None) is not None else (0, 0, 0)   # (else refused by the library)
        df = f if (f is None or hasattr(f, "ptr")) else DeviceVector(J.ctx, J.m, f)
        rows = B * mb
        dh = DeviceVector(J.ctx, rows)
        dse, dt, dck = [DeviceVector(J.ctx, rows) if f is not None else None for _ in range(3)]
        ds2 = DeviceVector(J.ctx, B) if f is not None else None
        info = np.zeros(max(B, 1), dtype=np.int32)
        check(lib().lsq_solver_leverage(self.h, J.h, _ptr(df), dh.ptr, _ptr(dse), _ptr(dt), _ptr(dck), _ptr(ds2),
                                        info.ctypes.data_as(_lib.c_ip)))
        if f is None:
            return Leverage(dh.get(), info=info[:B], nblocks=B, mb=mb)
        return Leverage(dh.get(), se=dse.get(), studentized=dt.get(), cook=dck.get(), s2=ds2.get(), info=info[:B], nblocks=B, mb=mb)

    def bordered_qr_leverage(self, f=None, block=None, A_local=None, A_shared=None):
        """lsq_bordered_qr_leverage at the values the bordered J holds now, from the factor of this BorderedQR() solver: a
        Leverage with `.rank` (the inner QR()'s) and `.block(b)`.  A_local = A_shared = None: the B * mb rows of J, `.q` = `.h`
        the leverages; with the residual `f` (DeviceVector or m host values) also `.se`, `.studentized`, `.cook` and `.s2` (one
        variance, sum(f.^2) / (m - n)).  `block`, A_local (p x nb, or nb values for one row) and A_shared (p x ng): p new rows of
        that block in the parameter space the handle means: `.q` the p quadratic forms and, with `f`, `.se` = sqrt(s2 q), the
        standard error of the prediction.  A zero or non-finite local column, or a rank-deficient border, raises
        RankDeficientException."""
        J = self.J
        B, mb, nb, ng = J.bordered if getattr(J, "bordered", None) is not None else (0, 0, 0, 0)   # (else refused by the library)
        df = f if (f is None or hasattr(f, "ptr")) else DeviceVector(J.ctx, J.m, f)
        fresh = A_local is not None or A_shared is not None
        dAb = dAg = None
        p = 0
        if A_local is not None:
            A_local = np.asarray(A_local, dtype=np.float64)
            A_local = A_local.reshape((1, -1)) if A_local.ndim == 1 else A_local
            if A_local.ndim != 2 or A_local.shape[1] != nb:
                raise DimensionMismatch(_lib.EDIM, "A_local has shape %s, expected (p, %d)" % (A_local.shape, nb))
            p = A_local.shape[0]
            dAb = DeviceVector(J.ctx, A_local.size, np.asfortranarray(A_local).reshape(-1, order="F"))
        if A_shared is not None:
            A_shared = np.asarray(A_shared, dtype=np.float64)
            A_shared = A_shared.reshape((1, -1)) if A_shared.ndim == 1 else A_shared
            if A_shared.ndim != 2 or A_shared.shape[1] != ng or (A_local is not None and A_shared.shape[0] != p):
                raise DimensionMismatch(_lib.EDIM, "A_shared has shape %s, expected (%s, %d)"
                                        % (A_shared.shape, p if A_local is not None else "p", ng))
            p = A_shared.shape[0]
            dAg = DeviceVector(J.ctx, A_shared.size, np.asfortranarray(A_shared).reshape(-1, order="F"))
        rows = p if fresh else B * mb
        own = not fresh and f is not None
        dq = DeviceVector(J.ctx, rows)
        dse = DeviceVector(J.ctx, rows) if f is not None else None
        dt = DeviceVector(J.ctx, rows) if own else None
        dck = DeviceVector(J.ctx, rows) if own else None
        s2, info = C.c_double(0.0), np.zeros(2, dtype=np.int32)
        check(lib().lsq_bordered_qr_leverage(self.h, J.h, -1 if block is None else int(block), _ptr(dAb), p, _ptr(dAg), p, p,
                                             _ptr(df), dq.ptr, _ptr(dse), _ptr(dt), _ptr(dck),
                                             C.byref(s2) if f is not None else None, info.ctypes.data_as(_lib.c_ip)))
        return Leverage(dq.get(), se=None if dse is None else dse.get(), studentized=None if dt is None else dt.get(),
                        cook=None if dck is None else dck.get(), s2=s2.value if f is not None else None, rank=int(info[1]),
                        nblocks=0 if fresh else B, mb=0 if fresh else mb)

    def stats(self):
        """lsq_solver_stats: give-ups of the co-residency fast paths and how many solves each stays paused."""
        g, p = (C.c_int * 4)(), (C.c_int * 4)()
        check(lib().lsq_solver_stats(self.h, g, p))
        names = ("chol_one_launch", "tri_pipeline", "qr_exchange", "cholqr_panel")
        return {k: {"giveups": g[i], "paused": p[i]} for i, k in enumerate(names)}

    def free(self):
        if self.h:
            lib().lsq_solver_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Covariance:
    """What lsq_solver_covariance returns, on the host: `.block(b)` the nb x nb covariance of block b's (local) parameters (a
    view), `.shared` the ng x ng covariance of a bordered handle's shared parameters (else None), `.stderr` the n standard
    errors in parameter order (or None), `.info` per block 0 or the 1-based column at which the block's Cholesky failed -- such
    a block is all NaN (block-diagonal handles only, else None)."""

    def __init__(self, nblocks, nb, ng, cov, stderr=None, info=None):
        self.nblocks, self.nb, self.ng = int(nblocks), int(nb), int(ng)
        self.cov = np.asarray(cov, dtype=np.float64)
        if self.cov.shape != (self.nblocks * self.nb * self.nb + self.ng * self.ng,):
            raise DimensionMismatch(_lib.EDIM, "covariance of %d blocks of %d parameters and %d shared ones has %d entries, got %s"
                                    % (self.nblocks, self.nb, self.ng, self.nblocks * self.nb * self.nb + self.ng * self.ng,
                                       self.cov.shape))
        self.stderr = None if stderr is None else np.asarray(stderr, dtype=np.float64)
        if self.stderr is not None and self.stderr.shape != (self.nblocks * self.nb + self.ng,):
            raise DimensionMismatch(_lib.EDIM, "stderr has shape %s, expected %d values"
                                    % (self.stderr.shape, self.nblocks * self.nb + self.ng))
        self.info = None if info is None else np.asarray(info, dtype=np.int32)

    def block(self, b):
        if not 0 <= b < self.nblocks:
            raise IndexError("block %d of %d" % (b, self.nblocks))
        k = self.nb * self.nb
        return self.cov[b * k:(b + 1) * k].reshape(self.nb, self.nb)

    @property
    def shared(self):
        if not self.ng:
            return None
        return self.cov[self.nblocks * self.nb * self.nb:].reshape(self.ng, self.ng)


def covariance(Jd, f=None, stderr=True):
    """Covariance of the parameters of a block-diagonal or bordered block-diagonal DeviceMatrix at the values it holds:
    creates a Cholesky() solver on it, calls AllocatedSolver.covariance and frees the solver."""
    sv = AllocatedSolver(Jd, Cholesky(), for_lm=True)
    try:
        return sv.covariance(f=f, stderr=stderr)
    finally:
        sv.free()


class BorderedCovariance(Covariance):
    """What lsq_bordered_qr_covariance returns, on the host: a Covariance (`.block(b)`, `.shared`, `.stderr`; `.cov` is None
    when it was not asked for, `.info` is None) with `.cross`, the (B nb) x ng local-shared cross-covariances -- the
    off-diagonal panel of the full covariance matrix in parameter order -- or None, `.cross_block(b)` its nb x ng rows of
    block b (a view), and `.rank`, the rank the inner QR() decided for the shared columns."""

    def __init__(self, nblocks, nb, ng, cov=None, stderr=None, cross=None, rank=None):
        size = int(nblocks) * int(nb) * int(nb) + int(ng) * int(ng)
        super().__init__(nblocks, nb, ng, np.zeros(size) if cov is None else cov, stderr)
        if cov is None:
            self.cov = None
        self.rank = rank
        if cross is None:
            self.cross = None
        else:
            cross = np.asarray(cross, dtype=np.float64)
            if cross.size != self.nblocks * self.nb * self.ng:
                raise DimensionMismatch(_lib.EDIM, "cross-covariance of %d x %d locals and %d shared parameters has %d entries, "
                                        "got %s" % (self.nblocks, self.nb, self.ng, self.nblocks * self.nb * self.ng, cross.shape))
            self.cross = cross.reshape((self.nblocks * self.nb, self.ng), order="F")

    def block(self, b):
        if self.cov is None:
            raise ValueError("the covariance blocks were not asked for (cov=False)")
        return super().block(b)

    @property
    def shared(self):
        if self.cov is None:
            return None
        return Covariance.shared.fget(self)

    def cross_block(self, b):
        if self.cross is None:
            raise ValueError("the cross-covariances were not asked for (cross=False)")
        if not 0 <= b < self.nblocks:
            raise IndexError("block %d of %d" % (b, self.nblocks))
        return self.cross[b * self.nb:(b + 1) * self.nb]


def bordered_qr_covariance(Jd, f=None, cov=True, stderr=True, cross=False):
    """Covariance of the parameters of a bordered block-diagonal DeviceMatrix at the values it holds, without squaring the
    condition number and for any ng: creates a BorderedQR() solver on it, calls AllocatedSolver.bordered_qr_covariance and frees
    the solver."""
    sv = AllocatedSolver(Jd, BorderedQR(), for_lm=True)
    try:
        return sv.bordered_qr_covariance(f=f, cov=cov, stderr=stderr, cross=cross)
    finally:
        sv.free()


class DenseCovariance:
    """What lsq_dense_covariance returns, on the host: `.cov` the n x n covariance s^2 inv(J'J) (symmetric to the bit),
    `.stderr` the n standard errors (or None), `.n` the number of parameters.  From lsq_sparse_covariance: `.cov` may be None
    (cov=False), and `.chol_path` names the factorisation that ran on J'J (else None)."""

    def __init__(self, n, cov, stderr=None, chol_path=None):
        self.n = int(n)
        self.chol_path = chol_path
        if cov is None:
            self.cov = None
        else:
            cov = np.asarray(cov, dtype=np.float64)
            if cov.size != self.n * self.n or cov.ndim > 2 or (cov.ndim == 2 and cov.shape != (self.n, self.n)):
                raise DimensionMismatch(_lib.EDIM, "covariance of %d parameters has %d x %d entries, got %s"
                                        % (self.n, self.n, self.n, cov.shape))
            self.cov = cov.reshape((self.n, self.n), order="F")
        self.stderr = None if stderr is None else np.asarray(stderr, dtype=np.float64)
        if self.stderr is not None and self.stderr.shape != (self.n,):
            raise DimensionMismatch(_lib.EDIM, "stderr has shape %s, expected %d values" % (self.stderr.shape, self.n))


def dense_covariance(Jd, f=None, stderr=True):
    """Covariance of the parameters of a dense DeviceMatrix at the values it holds: creates a Cholesky() solver on it, calls
    AllocatedSolver.dense_covariance and frees the solver."""
    sv = AllocatedSolver(Jd, Cholesky(), for_lm=True)
    try:
        return sv.dense_covariance(f=f, stderr=stderr)
    finally:
        sv.free()


def dense_qr_covariance(Jd, f=None, stderr=True):
    """The same from the QR() factor, which does not square the condition number: creates a QR() solver (for_lm=False) on the
    dense DeviceMatrix, calls AllocatedSolver.dense_qr_covariance and frees the solver."""
    sv = AllocatedSolver(Jd, QR(), for_lm=False)
    try:
        return sv.dense_qr_covariance(f=f, stderr=stderr)
    finally:
        sv.free()


class Leverage:
    """What lsq_dense_qr_leverage and lsq_solver_leverage return, on the host: `.q` (alias `.h`) the quadratic forms
    a' inv(J'J) a -- the leverages when the rows are J's own -- and, where the residual was given, `.se` the standard errors of
    the predictions, `.studentized` the internally studentized residuals, `.cook` Cook's distances (the latter two for J's own
    rows only) and `.s2` the residual variance (one value, or one per block); else None.  Dense: `.rank`, the rank the solve
    decided.  Block-diagonal: `.info` per block 0 or the 1-based column at which its factorisation failed (such a block is
    NaN), and `.block(b)` the same quantities for the mb rows of block b (views)."""

    def __init__(self, q, se=None, studentized=None, cook=None, s2=None, rank=None, info=None, nblocks=0, mb=0):
        self.q = np.asarray(q, dtype=np.float64)
        self.se, self.studentized, self.cook = se, studentized, cook
        self.s2, self.rank = s2, rank
        self.info = None if info is None else np.asarray(info, dtype=np.int32)
        self.nblocks, self.mb = int(nblocks), int(mb)

    @property
    def h(self):
        return self.q

    def block(self, b):
        if not 0 <= b < self.nblocks:
            raise IndexError("block %d of %d" % (b, self.nblocks))
        sl = slice(b * self.mb, (b + 1) * self.mb)
        cut = lambda v: None if v is None else v[sl]
        s2 = None if self.s2 is None else float(self.s2 if np.ndim(self.s2) == 0 else self.s2[b])    # (bordered: one variance)
        return Leverage(self.q[sl], se=cut(self.se), studentized=cut(self.studentized), cook=cut(self.cook), s2=s2,
                        rank=self.rank, info=None if self.info is None else self.info[b:b + 1])


def dense_qr_leverage(Jd, f=None, A=None):
    """Leverages (A=None) or prediction variances at new rows A of a dense DeviceMatrix at the values it holds: creates a QR()
    solver (for_lm=False) on it, calls AllocatedSolver.dense_qr_leverage and frees the solver."""
    sv = AllocatedSolver(Jd, QR(), for_lm=False)
    try:
        return sv.dense_qr_leverage(f=f, A=A)
    finally:
        sv.free()


def leverage(Jd, f=None):
    """Leverages of the B independent fits of a block-diagonal DeviceMatrix at the values it holds: creates a Cholesky() solver
    on it, calls AllocatedSolver.leverage and frees the solver."""
    sv = AllocatedSolver(Jd, Cholesky(), for_lm=True)
    try:
        return sv.leverage(f=f)
    finally:
        sv.free()


def bordered_qr_leverage(Jd, f=None, block=None, A_local=None, A_shared=None):
    """Leverages (no new rows) or prediction variances at new rows of one block of a bordered block-diagonal DeviceMatrix at the
    values it holds: creates a BorderedQR() solver on it, calls AllocatedSolver.bordered_qr_leverage and frees the solver."""
    sv = AllocatedSolver(Jd, BorderedQR(), for_lm=True)
    try:
        return sv.bordered_qr_leverage(f=f, block=block, A_local=A_local, A_shared=A_shared)
    finally:
        sv.free()


def sparse_covariance(Jd, f=None, cov=True, stderr=True):
    """Covariance of the parameters of a sparse (CSC) DeviceMatrix at the values it holds: creates an LSMR() solver on it, calls
    AllocatedSolver.sparse_covariance and frees the solver."""
    sv = AllocatedSolver(Jd, LSMR(), for_lm=True)
    try:
        return sv.sparse_covariance(f=f, cov=cov, stderr=stderr)
    finally:
        sv.free()


def sparse_gram(Jd, damp=None):
    """lsq_sparse_gram: J'J (+ diag(damp)) of a sparse (CSC) DeviceMatrix, formed on the device, as an n x n host array holding
    the upper triangle (the strict lower triangle, which the kernel leaves alone, is zeroed here)."""
    n = Jd.n if Jd.sparse else 0               # (any other handle is refused by the library, with its message)
    dd = damp if (damp is None or hasattr(damp, "ptr")) else DeviceVector(Jd.ctx, Jd.n, damp)
    dG = DeviceVector(Jd.ctx, n * n)
    check(lib().lsq_sparse_gram(Jd.h, _ptr(dd), dG.ptr))
    G = np.triu(dG.get().reshape((n, n), order="F"))
    dG.free()
    return G


# ------------------------------------------------------------------------------------------------
# robust losses and observation weights (include/lsqhip.h: lsq_loss_create)
# ------------------------------------------------------------------------------------------------
LOSSES = tuple(_lib.LOSS_KINDS)
_DBL_MAX = float(np.finfo(np.float64).max)


def _loss_arguments(loss, f_scale, sigma, m=None):
    """What lsq_loss_create checks, on the host: (loss, scale, sigma as a float64 array or None)."""
    if loss not in _lib.LOSS_KINDS:
        raise ArgumentError(_lib.EARG, "unknown loss %r (one of %s)" % (loss, ", ".join(LOSSES)))
    c = float(f_scale)
    if not 0.0 < c <= _DBL_MAX:
        raise ArgumentError(_lib.EARG, "the loss scale must be finite and positive (got %g)" % c)
    if sigma is None:
        return loss, c, None
    sg = np.ascontiguousarray(sigma, dtype=np.float64).reshape(-1)
    if m is not None and sg.size != m:
        raise DimensionMismatch(_lib.EDIM, "sigma has length %d, expected %d" % (sg.size, m))
    bad = np.flatnonzero(~((sg > 0.0) & (sg <= _DBL_MAX)))
    if bad.size:
        raise ArgumentError(_lib.EARG, "sigma must be finite and positive, entry %d is %g" % (bad[0], sg[bad[0]]))
    return loss, c, sg


def loss_transform(f, loss, f_scale=1.0, sigma=None):
    """The numpy twin of lsq_loss_eval and the normative statement of the transform: raw residuals f -> (rt, rowfactor) with
    z = f / sigma, a = |z| / c, rt = sign(z) c sqrt(rho(a^2)) and rowfactor = w / sigma, w = d rt / d z.  Every line is one
    IEEE operation per element in the order of the table in include/lsqhip.h, so "linear", "huber" and "soft_l1" have the
    device's bits ("cauchy" contains a log1p and agrees to rounding).  NaN and +-Inf pass through unchanged with w = 1 / 0
    ("linear": 1), signed zeros too."""
    f = np.asarray(f, dtype=np.float64)
    loss, c, sg = _loss_arguments(loss, f_scale, sigma, f.size)
    with np.errstate(all="ignore"):
        z = f / sg if sg is not None else f.copy()
        a = np.abs(z) / c
        rt, w = z.copy(), np.ones_like(z)
        if loss != "linear":
            fin = a <= _DBL_MAX
            w[~fin] = np.where(np.isnan(a[~fin]), 1.0, 0.0)
            if loss == "huber":
                sel = fin & (a > 1.0)
                ah = a[sel]
                q = np.where(ah > 2.0 ** 1022, 2.0 * np.sqrt(0.5 * ah), np.sqrt(2.0 * ah - 1.0))    # (2a would overflow)
                rt[sel] = np.copysign(c * q, z[sel])
                w[sel] = 1.0 / q
            elif loss == "soft_l1":
                sel = fin
                aa = a[sel]
                t = np.where(aa > 2.0 ** 500, aa, np.sqrt(1.0 + aa * aa))
                q = np.sqrt(2.0 / (t + 1.0))
                rt[sel] = z[sel] * q
                w[sel] = 1.0 / (t * q)
            else:
                sel = fin & (a >= 2.0 ** -27)
                aa = a[sel]
                big = aa > 2.0 ** 500
                L = np.where(big, 2.0 * np.log(aa), np.log1p(aa * aa))
                q = np.sqrt(L) / aa
                rt[sel] = z[sel] * q
                w[sel] = np.where(big, (1.0 / (aa * q)) / aa, 1.0 / ((1.0 + aa * aa) * q))
        rowfactor = w / sg if sg is not None else w
    return rt, rowfactor


def _scale_rows_host(J, rowfactor):
    """J <- diag(rowfactor) J in place on a host Jacobian: one product per stored value (lsq_mat_scale_rows' arithmetic)."""
    if _is_bordered(J) or _is_blockdiag(J):
        B, mb, nb = J.nblocks, J.mb, J.nb
        J.data[:B * mb * nb].reshape(B, nb, mb)[:] *= rowfactor.reshape(B, 1, mb)
        if _is_bordered(J):
            J.border[:, :] *= rowfactor[:, None]
    elif _is_sparse(J):
        J.data *= rowfactor[J.indices]
    else:
        J *= rowfactor[:, None]


def robust_twin(f_, g_, loss, f_scale=1.0, sigma=None):
    """(f_, g_) of the wrapped problem on the host, built on loss_transform: what lsq_loss_f / lsq_loss_g compute on the
    device.  The wrapped g_ calls g_, evaluates f_ itself at the same x (nothing is cached from an earlier f_ call) and
    scales the rows of J -- a dense array, a scipy.sparse CSC matrix in canonical order, a BlockDiagonal or a
    BorderedBlockDiagonal.  g_ = None gives (f_, None): central differences of the wrapped f_ are the Jacobian of the wrapped
    residual."""
    loss, c, sg = _loss_arguments(loss, f_scale, sigma)

    def rf_(out, x):
        f_(out, x)
        out[:] = loss_transform(out, loss, c, sg)[0]

    if g_ is None:
        return rf_, None

    def rg_(J, x):
        g_(J, x)
        raw = np.zeros(J.shape[0])
        f_(raw, x)
        _scale_rows_host(J, loss_transform(raw, loss, c, sg)[1])

    return rf_, rg_


class Loss:
    """The loss object of the C ABI (lsq_loss_create): kind, scale, m rows and a device copy of the sigmas.  `eval` is
    lsq_loss_eval on DeviceVectors; F / G are lsq_loss_f() / lsq_loss_g(), to be handed to a loop with `h` as the user
    pointer once set_problem has given it the inner callbacks."""

    def __init__(self, ctx, loss="linear", f_scale=1.0, m=None, sigma=None):
        if m is None:
            if sigma is None:
                raise ValueError("Loss needs m or sigma")
            m = len(sigma)
        self.ctx, self.loss, self.f_scale, self.m = ctx, loss, float(f_scale), int(m)
        ds = DeviceVector(ctx, self.m, sigma) if sigma is not None and self.m >= 1 else None
        h = C.c_void_p()
        try:      # (an unknown name goes to the library as -1: its refusal, its message)
            check(lib().lsq_loss_create(ctx.h, _lib.LOSS_KINDS.get(loss, -1), self.f_scale, self.m, _ptr(ds), C.byref(h)))
        finally:
            if ds is not None:
                ds.free()
        self.h = h
        self.F, self.G = lib().lsq_loss_f(), lib().lsq_loss_g()
        self._raw = DeviceVector(ctx, self.m)
        self._inner = None

    def set_problem(self, F, G=None):
        """lsq_loss_set_problem: the inner f! / g! as ctypes callbacks (G = None: none)."""
        self._inner = (F, G)        # (keeps the ctypes callbacks alive)
        check(lib().lsq_loss_set_problem(self.h, F, G if G is not None else _lib.G_CALLBACK(), None))

    def eval(self, f, rt=None, rowfactor=None, stats=False):
        """lsq_loss_eval: f (m raw residuals) -> rt (may be f itself) and rowfactor, DeviceVectors or None.  stats=True
        returns (sum(abs2, rt), rows with a > 1); otherwise nothing is read back."""
        for v in (f, rt, rowfactor):
            if v is not None and v.n != self.m:
                raise DimensionMismatch(_lib.EDIM, "vector has length %d, expected %d" % (v.n, self.m))
        st = (C.c_double * 2)() if stats else None
        check(lib().lsq_loss_eval(self.h, f.ptr, _ptr(rt), _ptr(rowfactor), st))
        return (float(st[0]), int(st[1])) if stats else None

    def transform(self, f):
        """eval on m host values: (rt, rowfactor, sum(abs2, rt), rows with a > 1)."""
        self._raw.set(f)
        drf = DeviceVector(self.ctx, self.m)
        ssr, out = self.eval(self._raw, self._raw, drf, stats=True)
        return self._raw.get(), drf.get(), ssr, out

    def free(self):
        if getattr(self, "h", None):
            lib().lsq_loss_destroy(self.h)
            self.h = None
            self._raw.free()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _new_loss(ctx, loss, f_scale, sigma, m):
    """The loss object of a loop call, or None for the defaults (the call is then exactly the one without these arguments)."""
    if loss == "linear" and sigma is None:
        return None
    loss, c, sg = _loss_arguments(loss, f_scale, sigma, m)
    return Loss(ctx, loss, c, m, sg)


def _loss_outliers(lossobj, host, dx):
    """h_stats[1] at the solution: one more evaluation of the raw f_ there."""
    if host._fcb(lossobj._raw.ptr, dx.ptr, None) != 0:
        raise host.err[-1]
    return lossobj.eval(lossobj._raw, stats=True)[1]


# ------------------------------------------------------------------------------------------------
# problem / result types
# ------------------------------------------------------------------------------------------------
class OptimizationState:
    def __init__(self, iteration, value, g_norm):
        self.iteration, self.value, self.g_norm = iteration, value, g_norm

    def __repr__(self):
        return "%6d   %14e   %14e" % (self.iteration, self.value, self.g_norm)


class LeastSquaresProblem:
    """types.jl:7-68.  J may be a numpy matrix (dense) or a scipy.sparse CSC matrix with a FIXED
    pattern whose `.data` g_ overwrites (test/nonlinearleastsquares.jl:47-86).
    autodiff="central_coloured" with a scipy.sparse J and no g_: coloured central differences on J's pattern, which must hold
    every (row, column) f_ depends on; `colouring` is one colour per column (validated: ArgumentError), None the greedy one."""

    def __init__(self, x=None, y=None, f_=None, g_=None, J=None, output_length=0, autodiff="central", colouring=None):
        if x is None:
            raise ValueError("initial x required")
        if f_ is None:
            raise ValueError("initial f! required")
        self.x = np.array(x, dtype=np.float64)
        if y is None:
            if output_length == 0:
                if J is None:
                    raise ValueError("specify J or output_length")
                output_length = J.shape[0]           # types.jl:46 (size(J, 1))
            y = np.zeros(output_length)
        self.y = np.asarray(y, dtype=np.float64)
        if J is None:
            J = np.zeros((len(self.y), len(self.x)), order="F")
        if type(J).__name__ == "DeviceOperator":
            if g_ is None:
                raise ValueError("a matrix-free Jacobian needs g_ (it updates the operator's own state)")
        elif _is_blockdiag(J) or _is_bordered(J):
            pass              # g_ writes J.data ([block][column][row], then the border) or the views J.block(b) / J.border
        elif _is_sparse(J):
            J = J.tocsc()
            J.sort_indices()  # g_ writes J.data in this (canonical CSC) order
        else:
            J = np.asfortranarray(J, dtype=np.float64)
        if len(self.x) != J.shape[1]:
            raise DimensionMismatch(_lib.EDIM, "x must have length size(J, 2)")
        if len(self.y) != J.shape[0]:
            raise DimensionMismatch(_lib.EDIM, "y must have length size(J, 1)")
        self.J = J
        self.f_ = f_
        self._fd_g = None
        self._fd_colouring = None
        if g_ is None:
            if autodiff == "central_coloured":
                if not _is_sparse(J):
                    raise ArgumentError(_lib.EARG, 'autodiff="central_coloured" needs a scipy.sparse J: its pattern is what is '
                                                   'coloured (dense and block Jacobians take autodiff="central")')
                if colouring is None:
                    colouring = greedy_colouring(J)[0]
                else:
                    colouring = _check_colouring(J, colouring)
                # as on block handles: the host twin for the Python-level loops; the native loops get a NULL g! and the
                # colouring is attached to the DeviceMatrix, as long as g_ is still this one
                self._fd_colouring = colouring
                g_ = self._fd_g = _sparse_colored_difference_jacobian(f_, len(self.y), colouring)
            elif autodiff == "central" and (_is_blockdiag(J) or _is_bordered(J)):
                # the coloured host twin for the Python-level loops; optimize_ / optimize_batched_ / an allocated problem hand
                # the native loops a NULL g! instead (central differences on the device) as long as g_ is still this one
                g_ = self._fd_g = _colored_difference_jacobian(f_, len(self.y))
            elif autodiff == "central":
                g_ = _central_difference_jacobian(f_, len(self.y))
            elif autodiff == "forward":
                raise NotImplementedError("autodiff=:forward (ForwardDiff) is off the hot path and "
                                          "never exercised by the reference's tests")
            else:
                raise ValueError("Invalid automatic differentiation method.")  # DomainError
        self.g_ = g_


def _central_difference_jacobian(f_, m):
    """FiniteDiff-style central differences (types.jl:55-58) -- host side, off the hot path."""
    eps3 = np.finfo(float).eps ** (1.0 / 3.0)

    def g_(J, x):
        if _is_sparse(J) or _is_blockdiag(J) or _is_bordered(J):
            raise ArgumentError(_lib.EARG, "autodiff Jacobians are dense only (types.jl:57)")
        fp, fm = np.zeros(m), np.zeros(m)
        xp = np.array(x, dtype=np.float64)
        for j in range(len(x)):
            h = max(eps3 * abs(x[j]), eps3)
            xj = xp[j]
            xp[j] = xj + h
            f_(fp, xp)
            xp[j] = xj - h
            f_(fm, xp)
            xp[j] = xj
            J[:, j] = (fp - fm) / (2 * h)

    return g_


FD_EPS3 = float.fromhex("0x1.965fea53d6e41p-18")     # np.finfo(float).eps ** (1 / 3), the literal of csrc/lsq_fd.hip


def _colored_difference_jacobian(f_, m):
    """The same central differences on a BlockDiagonal / BorderedBlockDiagonal J, by COLOURS: column c of every block is
    perturbed in one pair of evaluations (each entry with its own h), then every shared column on its own -- 2 nb (+ 2 ng)
    calls of f_ whatever the number of blocks is.  The host twin of lsq_fd_jacobian: the same f_ calls in the same order on
    the same full vectors, the same arithmetic per entry, so the same bits for the same f_."""
    eps3 = FD_EPS3

    def step(xj):   # max(eps3 * abs(xj), eps3) as Python's max evaluates it, elementwise
        a = eps3 * np.abs(xj)
        return np.where(eps3 > a, eps3, a)

    def g_(J, x):
        if not (_is_blockdiag(J) or _is_bordered(J)):
            raise ArgumentError(_lib.EARG, "coloured central differences need a BlockDiagonal or BorderedBlockDiagonal Jacobian")
        B, mb, nb, ng = J.nblocks, J.mb, J.nb, getattr(J, "ng", 0)
        x0 = np.array(x, dtype=np.float64)
        xp, xm = x0.copy(), x0.copy()
        fp, fm = np.zeros(m), np.zeros(m)
        blocks = J.data[:B * mb * nb].reshape(B, nb, mb)
        for c in range(nb):
            idx = np.arange(B) * nb + c
            xj = x0[idx]
            h = step(xj)
            xp[idx] = xj + h
            xm[idx] = xj - h
            f_(fp, xp)
            f_(fm, xm)
            xp[idx] = xj
            xm[idx] = xj
            blocks[:, c, :] = (fp - fm).reshape(B, mb) / (2 * h)[:, None]
        for k in range(ng):
            j = B * nb + k
            xj = x0[j]
            h = float(step(xj))
            xp[j] = xj + h
            xm[j] = xj - h
            f_(fp, xp)
            f_(fm, xm)
            xp[j] = xj
            xm[j] = xj
            J.data[B * mb * nb + k * m:B * mb * nb + (k + 1) * m] = (fp - fm) / (2 * h)

    return g_


def _csc_pattern(S):
    """(m, n, colptr, rowval) of a scipy.sparse matrix in canonical CSC order, int32."""
    S = S.tocsc()
    if not S.has_sorted_indices:
        S = S.sorted_indices()
    m, n = S.shape
    return m, n, np.ascontiguousarray(S.indptr, dtype=np.int32), np.ascontiguousarray(S.indices, dtype=np.int32)


def greedy_colouring(S):
    """lsq_csc_greedy_colouring on the pattern of the scipy.sparse S: (int32 array of n colours, ncolours).  First fit in
    natural column order: colour[j] is the smallest c >= 0 that no column k < j sharing a row with j holds; no two columns of
    one colour meet in a row, and the longest row is a lower bound on ncolours."""
    m, n, colptr, rowval = _csc_pattern(S)
    colour = np.zeros(n, dtype=np.int32)
    nc = C.c_int(0)
    check(lib().lsq_csc_greedy_colouring(m, n, colptr.ctypes.data_as(_lib.c_ip), rowval.ctypes.data_as(_lib.c_ip),
                                         colour.ctypes.data_as(_lib.c_ip), C.byref(nc)))
    return colour, nc.value


def _greedy_colouring_host(S):
    """The same algorithm in plain Python (the host twin of lsq_csc_greedy_colouring): stamp array over a row view."""
    m, n, colptr, rowval = _csc_pattern(S)
    R = _sp.csr_matrix((np.ones(len(rowval)), rowval, colptr), shape=(n, m)).tocsc()     # (the transpose's CSC = our CSR)
    R.sort_indices()
    rptr, ridx = R.indptr, R.indices
    colour = np.zeros(n, dtype=np.int32)
    stamp = np.full(n + 1, -1, dtype=np.int64)
    nc = 0
    for j in range(n):
        for i in rowval[colptr[j]:colptr[j + 1]]:
            for k in ridx[rptr[i]:rptr[i + 1]]:
                if k >= j:
                    break
                stamp[colour[k]] = j
        c = 0
        while stamp[c] == j:
            c += 1
        colour[j] = c
        nc = max(nc, c + 1)
    return colour, nc


def _check_colouring(S, colouring):
    """What lsq_mat_set_fd_colouring checks, on the host: one colour >= 0 per column, every colour 0 .. max used, no row with
    two columns of one colour.  Returns the colours as an int32 array; ArgumentError otherwise."""
    m, n, colptr, rowval = _csc_pattern(S)
    a = np.asarray(colouring)
    if a.ndim != 1 or a.size != n or a.dtype.kind not in "iu":
        raise ArgumentError(_lib.EARG, "a colouring has one integer colour per column (%d), got %r" % (n, a.shape))
    a = a.astype(np.int64)
    if n == 0:
        return a.astype(np.int32)
    if a.min() < 0:
        j = int(np.argmin(a))
        raise ArgumentError(_lib.EARG, "column %d has the negative colour %d" % (j, a[j]))
    nc = int(a.max()) + 1
    used = np.bincount(a, minlength=nc) if nc <= n else np.zeros(1)
    if nc > n or np.any(used == 0):
        raise ArgumentError(_lib.EARG, "the colours must be 0 .. ncolours-1 without a gap (largest colour %d)" % (nc - 1))
    # (row, colour) of every stored entry: a valid colouring has no pair twice
    col_of = np.repeat(np.arange(n), np.diff(colptr))
    key = rowval.astype(np.int64) * nc + a[col_of]
    order = np.argsort(key, kind="stable")
    dup = np.flatnonzero((key[order][1:] == key[order][:-1]) & (col_of[order][1:] != col_of[order][:-1]))
    if dup.size:
        p, q = order[dup[0]], order[dup[0] + 1]
        raise ArgumentError(_lib.EARG, "row %d holds columns %d and %d, both of colour %d" % (rowval[p], col_of[p], col_of[q],
                                                                                             a[col_of[p]]))
    return a.astype(np.int32)


def _sparse_colored_difference_jacobian(f_, m, colour):
    """Coloured central differences on a scipy.sparse J with a fixed pattern: all columns of one colour are perturbed in one
    pair of evaluations (each with its own h), and every stored entry (i, j) is (f+[i] - f-[i]) / (2 h_j).  2 ncolours calls
    of f_.  The host twin of lsq_fd_jacobian on a coloured CSC handle: the same f_ calls in the same order on the same full
    vectors, the same arithmetic per entry, J.data written in canonical CSC order.  The pattern must hold every
    (row, column) f_ depends on."""
    eps3 = FD_EPS3
    colour = np.asarray(colour, dtype=np.int64)
    nc = int(colour.max()) + 1 if colour.size else 0
    members = [np.flatnonzero(colour == c) for c in range(nc)]

    def step(xj):   # max(eps3 * abs(xj), eps3) as Python's max evaluates it, elementwise
        a = eps3 * np.abs(xj)
        return np.where(eps3 > a, eps3, a)

    def g_(J, x):
        if not _is_sparse(J) or J.format != "csc":
            raise ArgumentError(_lib.EARG, "coloured central differences on a pattern need a scipy.sparse CSC Jacobian")
        if J.shape[1] != colour.size:
            raise ArgumentError(_lib.EARG, "the colouring has %d columns, J has %d" % (colour.size, J.shape[1]))
        colptr, rowval = J.indptr, J.indices
        col_of = np.repeat(np.arange(J.shape[1]), np.diff(colptr))
        x0 = np.array(x, dtype=np.float64)
        xp, xm = x0.copy(), x0.copy()
        fp, fm = np.zeros(m), np.zeros(m)
        h_all = step(x0)
        ecol = colour[col_of]                                  # the stored entries, grouped by the colour of their column
        order = np.argsort(ecol, kind="stable")
        cuts = np.searchsorted(ecol[order], np.arange(nc + 1))
        for c, idx in enumerate(members):
            xj = x0[idx]
            h = h_all[idx]
            xp[idx] = xj + h
            xm[idx] = xj - h
            f_(fp, xp)
            f_(fm, xm)
            xp[idx] = xj
            xm[idx] = xj
            ks = order[cuts[c]:cuts[c + 1]]
            J.data[ks] = (fp[rowval[ks]] - fm[rowval[ks]]) / (2 * h_all[col_of[ks]])

    return g_


def _device_fd(nls):
    """Does this problem take its Jacobian from the device's central differences (g_ was left to the default on a block
    handle or to autodiff="central_coloured" on a sparse one, and is still that default)?"""
    twin = getattr(nls, "_fd_g", None)
    return twin is not None and nls.g_ is twin


def fd_jacobian_(Jd, x, f_):
    """lsq_fd_jacobian: the values of the DeviceMatrix Jd <- central differences of the host f_(out, x) at x (a DeviceVector,
    or n host values), colour by colour on the device; every layout of the handle is refreshed.  Dense, block-diagonal and
    bordered handles, and a sparse one with a colouring attached (DeviceMatrix.set_fd_colouring); anything else raises
    ArgumentError.  An exception raised by f_ is re-raised here."""
    ctx = Jd.ctx
    dx = x if hasattr(x, "ptr") else DeviceVector(ctx, Jd.n, x)
    if dx.n != Jd.n:
        raise DimensionMismatch(_lib.EDIM, "x has length %d, expected %d" % (dx.n, Jd.n))
    xh, yh, err = np.zeros(Jd.n), np.zeros(Jd.m), []

    def _fcb(d_out, d_x, _):
        L = lib()
        try:
            check(L.lsq_d2h(ctx.h, xh.ctypes.data_as(C.c_void_p), d_x, Jd.n * 8))
            f_(yh, xh)
            check(L.lsq_h2d(ctx.h, d_out, yh.ctypes.data_as(C.c_void_p), Jd.m * 8))
            return 0
        except Exception as e:  # surfaced after the C call returns
            err.append(e)
            return 1

    F = _lib.F_CALLBACK(_fcb)
    st = lib().lsq_fd_jacobian(ctx.h, Jd.h, dx.ptr, F, None)
    if err:
        raise err[0]
    check(st)
    return Jd


class LeastSquaresResult:
    """types.jl:220-269"""

    def __repr__(self):
        ok = self.x_converged or self.f_converged or self.g_converged
        return ("Results of Optimization Algorithm\n * Status: %s\n\n * Candidate solution\n"
                "    Final objective value:     %.6e\n\n * Found with\n    Algorithm:     %s\n\n"
                " * Convergence measures\n    |x - x'|               %s %.1e\n"
                "    |f(x) - f(x')| / |f(x)| %s %.1e\n    |g(x)|                 %s %.1e\n\n"
                " * Work counters\n    Iterations:    %d\n    f(x) calls:    %d\n"
                "    J(x) calls:    %d\n    mul! calls:    %d\n" % (
                    "success" if ok else "failure (reached maximum number of iterations)",
                    self.ssr, self.optimizer, "<=" if self.x_converged else "!<=", self.x_tol,
                    "<=" if self.f_converged else "!<=", self.f_tol,
                    "<=" if self.g_converged else "!<=", self.g_tol,
                    self.iterations, self.f_calls, self.g_calls, self.mul_calls))


def converged(r):
    return r.x_converged or r.f_converged or r.g_converged


class _HostCallbacks:
    """f! / g! of a host-side problem as the C callbacks of lsq_optimize / lsq_optimize_batched (device pointers in, numpy out).
    Host-side g!: the Jacobian values live in PAGE-LOCKED memory for the duration of the solve -- g! writes them there
    directly (a sparse J gets its .data rebound to the pinned array, a dense J is handed over as a pinned column-major
    view) and the upload after every g!(J, x) is asynchronous (lsq_mat_set_values_async): no staging copy, no blocked
    host, PCIe rate instead of the pageable-copy rate.  SURVEY 8f-1; levenberg_marquardt.jl:77-81 is where the upload sits.
    bind() rebinds, release() (in a finally) hands J.data back in ordinary memory; exceptions raised inside f! / g! are
    collected in .err and surfaced by the caller after the C call has returned."""

    def __init__(self, ctx, nls, Jd, stage=None):
        self.ctx, self.nls, self.Jd = ctx, nls, Jd
        # central differences on the device: the loop gets a NULL g! (.G), nothing is staged or uploaded, and the values are
        # downloaded into nls.J.data once, at the end (fetch_jacobian)
        self.device_fd = _device_fd(nls)
        colouring = getattr(nls, "_fd_colouring", None)
        if self.device_fd and colouring is not None and getattr(Jd, "_fd_attached", None) is not colouring:
            Jd.set_fd_colouring(colouring)       # (a sparse J with autodiff="central_coloured"; once per handle)
            Jd._fd_attached = colouring
        self.n, self.m = len(nls.x), len(nls.y)
        self.is_op = isinstance(nls.J, DeviceOperator)
        self.own_stage = stage is None
        self.given_stage = stage
        self.stage = None
        self.J_user = nls.J
        self.data_user = None
        self.J_for_g = None
        self.err = []
        self.xh, self.yh = np.zeros(self.n), np.zeros(self.m)
        self.F = _lib.F_CALLBACK(self._fcb)
        self.G = _lib.G_CALLBACK() if self.device_fd else _lib.G_CALLBACK(self._gcb)

    def bind(self):
        # (called inside the caller's try: whatever happens after the rebinding, release() hands J.data back)
        if self.is_op or self.device_fd:
            return
        nls, Jd = self.nls, self.Jd
        self.stage = self.given_stage if self.given_stage is not None else PinnedBuffer(self.ctx, Jd.nnz)
        if Jd.sparse:
            self.data_user = nls.J.data
            np.copyto(self.stage.array, self.data_user)
            nls.J.data = self.stage.array
            self.J_for_g = nls.J
        else:
            self.J_for_g = self.stage.array.reshape((self.m, self.n), order="F")
            np.copyto(self.J_for_g, nls.J)

    def _fcb(self, d_out, d_x, _):
        L = lib()
        try:
            check(L.lsq_d2h(self.ctx.h, self.xh.ctypes.data_as(C.c_void_p), d_x, self.n * 8))
            self.nls.f_(self.yh, self.xh)
            check(L.lsq_h2d(self.ctx.h, d_out, self.yh.ctypes.data_as(C.c_void_p), self.m * 8))
            return 0
        except Exception as e:  # surfaced after the C call returns
            self.err.append(e)
            return 1

    def _gcb(self, Jh, d_x, _):
        L = lib()
        nls, Jd, stage = self.nls, self.Jd, self.stage
        try:
            check(L.lsq_d2h(self.ctx.h, self.xh.ctypes.data_as(C.c_void_p), d_x, self.n * 8))
            if self.is_op:   # g! updates the operator's own state; nothing to upload
                nls.g_(nls.J, self.xh)
                return 0
            Jd.upload_wait()            # (the previous upload has long finished; g! is about to overwrite its source)
            nls.g_(self.J_for_g, self.xh)
            if Jd.sparse and nls.J.data is not stage.array:     # g! replaced J.data instead of writing into it
                np.copyto(stage.array, nls.J.data)
                nls.J.data = stage.array
            Jd.set_values_async(stage)
            return 0
        except Exception as e:
            self.err.append(e)
            return 1

    def fetch_jacobian(self):
        """device_fd: nls.J holds the Jacobian of the last evaluation (nothing was staged: release() has nothing to copy)."""
        if self.device_fd:
            self.nls.J.data[:] = self.Jd.values()

    def fetch_scaled_jacobian(self):
        """With a loss the handle holds diag(w / sigma) J, the staging buffer the raw values of the last g!: nls.J gets the
        handle's (after release(), which has handed J.data back)."""
        if self.is_op:
            return
        v = self.Jd.values()
        if self.Jd.sparse:
            self.nls.J.data[:] = v
        else:
            self.nls.J[:, :] = v.reshape((self.m, self.n), order="F")

    def release(self):
        stage = self.stage
        if stage is None:
            return
        # hand the values back in ordinary memory before the pinned buffer can go away
        self.Jd.upload_wait()
        if self.Jd.sparse:
            if self.data_user is not None:
                self.data_user[:] = stage.array
                self.nls.J.data = self.data_user
        elif self.J_for_g is not None:
            np.copyto(self.J_user, self.J_for_g)
        if self.own_stage:
            stage.free()
        self.stage = None


def _run_native(ctx, optimizer_kind, solver_kind, Jd, dx, dy, fcb, gcb, user, x_tol, f_tol, g_tol,
                iterations, delta, lower, upper, trace, n, allreduce=None, preconditioner=None, row_allreduce=None,
                row_allreduce_user=None, global_rows=0, general_preconditioner=None):
    L = lib()
    opt = _lib.Options()
    L.lsq_options_default(C.byref(opt))
    opt.x_tol, opt.f_tol, opt.g_tol = float(x_tol), float(f_tol), float(g_tol)
    opt.iterations = int(iterations)
    opt.delta = float(delta) if delta is not None else -1.0
    keep = []
    if lower is not None and len(lower):
        lo = np.ascontiguousarray(lower, dtype=np.float64)
        if len(lo) != n:
            raise ArgumentError(_lib.EARG, "Bounds must either be empty or of the same length as "
                                           "the number of parameters.")
        opt.h_lower = lo.ctypes.data_as(_lib.c_dp)
        keep.append(lo)
    if upper is not None and len(upper):
        hi = np.ascontiguousarray(upper, dtype=np.float64)
        if len(hi) != n:
            raise ArgumentError(_lib.EARG, "Bounds must either be empty or of the same length as "
                                           "the number of parameters.")
        opt.h_upper = hi.ctypes.data_as(_lib.c_dp)
        keep.append(hi)
    if allreduce is not None:
        if hasattr(allreduce, "callback"):      # an exchange served in C (sharding.RcclScalarExchange): function + handle
            if hasattr(allreduce, "reset"):
                allreduce.reset()               # (the protocol state is per run: include/lsqrccl.h)
            opt.allreduce = allreduce.callback
            opt.allreduce_user = allreduce.user
        else:                                   # a ctypes callback (sharding.make_allreduce_callback)
            opt.allreduce = allreduce
        keep.append(allreduce)
    if preconditioner is not None:
        opt.preconditioner = preconditioner
        keep.append(preconditioner)
    if general_preconditioner is not None:     # LSMR(preconditioner!, P) with a general P: (update_cb, ldiv_cb)
        opt.precond_update, opt.precond_ldiv = general_preconditioner
        keep.append(general_preconditioner)
    if row_allreduce is not None:       # row-sharded single problem (lsq_options.row_allreduce; rowshard.py)
        opt.row_allreduce = row_allreduce
        opt.row_allreduce_user = row_allreduce_user
        opt.global_rows = int(global_rows)
        keep.append(row_allreduce)
    tr = None
    if trace:
        cap = int(iterations)
        tr = dict(ssr=np.zeros(cap), gnorm=np.zeros(cap), delta=np.zeros(cap), rho=np.zeros(cap),
                  inner=np.zeros(cap, dtype=np.int32), accept=np.zeros(cap, dtype=np.int32),
                  x=np.zeros((cap, n)))
        opt.trace_cap = cap
        opt.trace_ssr = tr["ssr"].ctypes.data_as(_lib.c_dp)
        opt.trace_gnorm = tr["gnorm"].ctypes.data_as(_lib.c_dp)
        opt.trace_delta = tr["delta"].ctypes.data_as(_lib.c_dp)
        opt.trace_rho = tr["rho"].ctypes.data_as(_lib.c_dp)
        opt.trace_inner = tr["inner"].ctypes.data_as(_lib.c_ip)
        opt.trace_accept = tr["accept"].ctypes.data_as(_lib.c_ip)
        opt.trace_x = tr["x"].ctypes.data_as(_lib.c_dp)
    res = _lib.Result()
    st = L.lsq_optimize(ctx.h, optimizer_kind, solver_kind, Jd.h, dx.ptr, dy.ptr, fcb, gcb, user,
                        C.byref(opt), C.byref(res))
    if tr is not None:
        k = res.iterations
        tr = {key: v[:k].copy() for key, v in tr.items()}
    return st, res, tr


def optimize_(nls, optimizer=None, x_tol=1e-8, f_tol=1e-8, g_tol=1e-8, iterations=1000, delta=None,
              store_trace=False, show_trace=False, show_every=1, lower=(), upper=(), ctx=None,
              full_trace=False, row_allreduce=None, global_rows=0, loss="linear", f_scale=1.0, sigma=None):
    """optimize!(nls, optimizer; kwargs...)  -- types.jl:207-209 then
    levenberg_marquardt.jl:39-144 / dogleg.jl:41-203.  Mutates nls.x, nls.y, nls.J in place.
    loss ("linear", "huber", "soft_l1", "cauchy"), f_scale and sigma (m per-point uncertainties): the loop minimises the robust,
    weighted cost through the wrapped problem of include/lsqhip.h (lsq_loss_create) -- f_ / g_ stay the raw residual and its
    Jacobian; afterwards nls.y holds the wrapped residual, nls.J the wrapped Jacobian, r.ssr = f_scale^2 sum(rho), and the
    result carries loss, f_scale and outliers (rows with |f / sigma| > f_scale at the solution).  With the defaults nothing of
    this exists.  An allocated problem takes them at allocation.
    On a BorderedBlockDiagonal Jacobian Cholesky() without an optimizer means LevenbergMarquardt(Cholesky()), and
    Dogleg(Cholesky()) raises ArgumentError (it does not exist there); LevenbergMarquardt / Dogleg with LSMR() run as on any
    sparse Jacobian."""
    allocated = nls if isinstance(nls, LeastSquaresProblemAllocated) else None
    if allocated is not None:
        # optimize!(nls::LeastSquaresProblemAllocated; kwargs...): buffers, solver and optimizer were chosen at
        # allocation (types.jl:141-160); nothing is allocated here, on the host or on the device
        if optimizer is not None:
            raise TypeError("an allocated problem carries its optimizer (types.jl:152-157)")
        if loss != "linear" or sigma is not None or f_scale != 1.0:
            raise TypeError("an allocated problem carries its loss: give loss, f_scale and sigma to LeastSquaresProblemAllocated")
        ctx, optimizer, solver = allocated.ctx, allocated.optimizer, allocated.solver
    else:
        solver = default_solver(optimizer.solver if optimizer is not None else None, nls.J)   # (refusals need no device)
        optimizer = default_optimizer(optimizer, solver, nls.J)
        ctx = ctx or default_context()
    n, m = len(nls.x), len(nls.y)
    if allocated is None and (loss != "linear" or sigma is not None):
        loss, f_scale, sigma = _loss_arguments(loss, f_scale, sigma, m)      # (refusals before anything is allocated)
    is_op = isinstance(nls.J, DeviceOperator)
    if allocated is not None:
        Jd, dx, dy = allocated._Jd, allocated._dx, allocated._dy
        dx.set(nls.x)
        dy.set(nls.y)
    else:
        Jd = nls.J if is_op else DeviceMatrix(ctx, nls.J)
        dx, dy = DeviceVector(ctx, n, nls.x), DeviceVector(ctx, m, nls.y)
    host = _HostCallbacks(ctx, nls, Jd, allocated._stage if allocated is not None else None)
    err = host.err
    F, G, user = host.F, host.G, None
    lossobj = allocated._loss if allocated is not None else _new_loss(ctx, loss, f_scale, sigma, m)
    if lossobj is not None:     # the host callbacks become the inner problem; the loop gets the wrapper (a null g! stays null)
        lossobj.set_problem(host.F, None if host.device_fd else host.G)
        F, user = lossobj.F, lossobj.h
        G = host.G if host.device_fd else lossobj.G
    tracing = store_trace or show_trace or full_trace
    st = res = tr = None
    try:
        host.bind()
        pc = gpc = None
        if getattr(solver, "P", None) is not None:
            gpc = _general_precond_trampolines(solver, ctx, Jd)
        elif getattr(solver, "preconditioner", None) is not None:
            pc = _precond_trampoline(solver.preconditioner, ctx, Jd)
        # row_allreduce: a rowshard.RcclRowAllreduce / HostStagedRowAllreduce -- nls then holds this rank's ROWS of one
        # larger problem (J, y local; x replicated), SURVEY 8f-4
        st, res, tr = _run_native(ctx, optimizer.kind, solver.kind, Jd, dx, dy, F, G, user, x_tol, f_tol,
                                  g_tol, iterations, delta, lower, upper, tracing, n, preconditioner=pc,
                                  general_preconditioner=gpc,
                                  row_allreduce=row_allreduce.callback if row_allreduce is not None else None,
                                  row_allreduce_user=row_allreduce.user if row_allreduce is not None else None,
                                  global_rows=global_rows)
    finally:
        host.release()
        if st is not None:
            host.fetch_jacobian()
            if lossobj is not None:
                host.fetch_scaled_jacobian()
            # optimize! mutates nls.x / nls.y in place (levenberg_marquardt.jl:46): when an iteration throws
            # (RankDeficientException, IsFiniteException, ...) they hold that iteration's iterate, as in the reference
            nls.x[:] = dx.get()
            nls.y[:] = dy.get()
    try:
        if err:
            raise err[0]
        if st == _lib.ENONFINITE:
            e = _lib.IsFiniteException(st, lib().lsq_last_error().decode())
            e.indices = [res.bad_index]
            raise e
        check(st)
        outliers = _loss_outliers(lossobj, host, dx) if lossobj is not None else None
    finally:
        if lossobj is not None and allocated is None:
            lossobj.free()
    r = LeastSquaresResult()
    if lossobj is not None:
        r.loss, r.f_scale, r.outliers = lossobj.loss, lossobj.f_scale, outliers
    r.optimizer = optimizer.name
    r.minimizer = nls.x
    r.ssr = float(res.ssr)
    r.iterations = res.iterations
    r.converged = bool(res.converged)
    r.x_converged, r.f_converged, r.g_converged = bool(res.x_converged), bool(res.f_converged), bool(res.g_converged)
    r.x_tol, r.f_tol, r.g_tol = float(x_tol), float(f_tol), float(g_tol)
    r.f_calls, r.g_calls, r.mul_calls = res.f_calls, res.g_calls, res.mul_calls
    r.jacobian = nls.J
    r.seconds = res.seconds
    r.trace = tr
    states = []
    if tracing and tr is not None:
        # levenberg_marquardt.jl:70 / dogleg.jl:74: state 0 = (0, ssr(x0), Inf), then one state per iteration
        states.append(OptimizationState(0, float(res.ssr0), float("inf")))
        for k in range(res.iterations):
            states.append(OptimizationState(k + 1, tr["ssr"][k], tr["gnorm"][k]))
        if show_trace:
            print("Iter     Function value   Gradient norm ")
            print("------   --------------   --------------")
            for s_ in states:
                if s_.iteration % show_every == 0:
                    print(s_)
    r.tr = states if store_trace else []
    if not is_op and allocated is None:
        Jd.free()
    return r


# ------------------------------------------------------------------------------------------------
# B independent fits on a block-diagonal Jacobian: one trust region per block (lsq_optimize_batched)
# ------------------------------------------------------------------------------------------------
_BATCHED_INT = ("iterations", "converged", "x_converged", "f_converged", "g_converged", "f_calls", "g_calls", "mul_calls",
                "status", "info")


class BatchedResult:
    """Result of optimize_batched_: arrays of length B named as the fields of LeastSquaresResult (ssr, iterations, converged,
    x_converged, f_converged, g_converged, f_calls, g_calls, mul_calls), plus `status` / `info` (the lsq_status of each fit and
    its block-local column / rank / index, -1 when there is none), `ssr0`, the stacked `minimizer`, `outer_iterations`,
    `seconds` and, when requested, `trace` (ssr / gnorm / delta / rho / accept: (cap, B); x: (cap, n); row k of block b is only
    meaningful for k < iterations[b]).  block(b) is fit b as a LeastSquaresResult."""

    def __init__(self, nblocks, mb, nb, optimizer="LevenbergMarquardt", x_tol=1e-8, f_tol=1e-8, g_tol=1e-8):
        self.nblocks, self.mb, self.nb = int(nblocks), int(mb), int(nb)
        self.optimizer = optimizer
        self.x_tol, self.f_tol, self.g_tol = float(x_tol), float(f_tol), float(g_tol)
        B = self.nblocks
        self.ssr, self.ssr0 = np.zeros(B), np.zeros(B)
        for k in _BATCHED_INT:
            setattr(self, k, np.zeros(B, dtype=np.int32))
        self.info[:] = -1
        self.minimizer = np.zeros(B * self.nb)
        self.outer_iterations, self.seconds = 0, 0.0
        self.trace = None

    def block(self, b):
        if not 0 <= b < self.nblocks:
            raise IndexError("block %d of %d" % (b, self.nblocks))
        r = LeastSquaresResult()
        r.optimizer = self.optimizer
        r.minimizer = self.minimizer[b * self.nb:(b + 1) * self.nb]
        r.ssr, r.ssr0 = float(self.ssr[b]), float(self.ssr0[b])
        r.iterations = int(self.iterations[b])
        r.converged = bool(self.converged[b])
        r.x_converged, r.f_converged, r.g_converged = bool(self.x_converged[b]), bool(self.f_converged[b]), bool(self.g_converged[b])
        r.x_tol, r.f_tol, r.g_tol = self.x_tol, self.f_tol, self.g_tol
        r.f_calls, r.g_calls, r.mul_calls = int(self.f_calls[b]), int(self.g_calls[b]), int(self.mul_calls[b])
        r.status, r.info = int(self.status[b]), int(self.info[b])
        r.trace = None
        if self.trace is not None:
            k = min(r.iterations, self.trace["ssr"].shape[0])
            r.trace = {key: self.trace[key][:k, b].copy() for key in ("ssr", "gnorm", "delta", "rho", "accept")}
            r.trace["x"] = self.trace["x"][:k, b * self.nb:(b + 1) * self.nb].copy()
            # solves per iteration: Cholesky() and BlockQR() are one, and Dogleg reuses its steps after a refused one (dogleg.jl:81)
            inner = np.ones(k, dtype=np.int32)
            if self.optimizer == "Dogleg" and k > 1:
                inner[1:] = r.trace["accept"][:k - 1]
            r.trace["inner"] = inner
        return r


def _batched_arguments(J, optimizer, n, lower, upper):
    """Everything optimize_batched_ can refuse before a device call; returns (optimizer, solver)."""
    if _is_bordered(J):
        raise ArgumentError(_lib.EARG, "optimize_batched_ does not take a BorderedBlockDiagonal Jacobian: the shared columns "
                                       "couple the blocks, so there is no trust region per block. Use optimize_")
    if not _is_blockdiag(J):
        raise ArgumentError(_lib.EARG, "optimize_batched_ needs a BlockDiagonal Jacobian: one trust region per block "
                                       "needs the block shape")
    if optimizer is None:
        optimizer = LevenbergMarquardt(Cholesky())
    solver = optimizer.solver if optimizer.solver is not None else Cholesky()
    if isinstance(solver, QR):
        raise ArgumentError(_lib.EARG, "solver QR() is not available for sparse Jacobians. "
                                       "Choose between Cholesky() and LSMR()")
    if isinstance(solver, Schur):
        raise ArgumentError(_lib.EARG, "optimize_batched_: Schur() solves the one coupled system of a BorderedBlockDiagonal "
                                       "Jacobian, there is no trust region per block in it. Use optimize_ with "
                                       "LevenbergMarquardt(Schur())")
    if isinstance(solver, BorderedQR):
        raise ArgumentError(_lib.EARG, "optimize_batched_: BorderedQR() solves the one coupled system of a "
                                       "BorderedBlockDiagonal Jacobian, there is no trust region per block in it. Use "
                                       "optimize_ with LevenbergMarquardt(BorderedQR())")
    if isinstance(solver, LSMR):
        raise ArgumentError(_lib.EARG, "optimize_batched_: LSMR() is not available per block (an iterative solve per block "
                                       "is a different loop). Use Cholesky(), or optimize_ for one trust region over the "
                                       "stacked problem")
    if isinstance(solver, BlockQR):
        default_solver(solver, J)
    elif J.nb > 64:
        raise ArgumentError(_lib.EARG, "optimize_batched_: Cholesky() per block needs blocks of at most 64 columns "
                                       "(got nb = %d)" % J.nb)
    for bound in (lower, upper):
        if bound is not None and len(bound) and len(bound) != n:
            raise ArgumentError(_lib.EARG, "Bounds must either be empty or of the same length as "
                                           "the number of parameters.")
    return default_optimizer(optimizer, solver), solver


def _run_native_batched(ctx, optimizer_kind, solver_kind, Jh, shape, dx, dy, fcb, gcb, user, x_tol, f_tol, g_tol, iterations,
                        delta, lower, upper, trace, optimizer_name, options_hook=None):
    """lsq_optimize_batched on device buffers; returns (status, BatchedResult without its minimizer)."""
    L = lib()
    B, mb, nb = shape
    n = B * nb
    opt = _lib.Options()
    L.lsq_options_default(C.byref(opt))
    opt.x_tol, opt.f_tol, opt.g_tol = float(x_tol), float(f_tol), float(g_tol)
    opt.iterations = int(iterations)
    opt.delta = float(delta) if delta is not None else -1.0
    keep = []
    for name, bound in (("h_lower", lower), ("h_upper", upper)):
        if bound is not None and len(bound):
            v = np.ascontiguousarray(bound, dtype=np.float64)
            setattr(opt, name, v.ctypes.data_as(_lib.c_dp))
            keep.append(v)
    if options_hook is not None:
        options_hook(opt)
    r = BatchedResult(B, mb, nb, optimizer_name, x_tol, f_tol, g_tol)
    res = _lib.BatchedResult()
    res.ssr, res.ssr0 = r.ssr.ctypes.data_as(_lib.c_dp), r.ssr0.ctypes.data_as(_lib.c_dp)
    for k in _BATCHED_INT:
        setattr(res, k, getattr(r, k).ctypes.data_as(_lib.c_ip))
    tr = None
    if trace:
        cap = int(iterations)
        tr = dict(ssr=np.zeros((cap, B)), gnorm=np.zeros((cap, B)), delta=np.zeros((cap, B)), rho=np.zeros((cap, B)),
                  accept=np.zeros((cap, B), dtype=np.int32), x=np.zeros((cap, n)))
        res.trace_cap = cap
        for key in ("ssr", "gnorm", "delta", "rho", "x"):
            setattr(res, "trace_" + key, tr[key].ctypes.data_as(_lib.c_dp))
        res.trace_accept = tr["accept"].ctypes.data_as(_lib.c_ip)
    st = L.lsq_optimize_batched(ctx.h, optimizer_kind, solver_kind, Jh, dx.ptr, dy.ptr, fcb, gcb, user, C.byref(opt),
                                C.byref(res))
    r.outer_iterations, r.seconds = int(res.outer_iterations), float(res.seconds)
    if tr is not None:
        k = r.outer_iterations
        r.trace = {key: v[:k].copy() for key, v in tr.items()}
    return st, r


def optimize_batched_(nls, optimizer=None, x_tol=1e-8, f_tol=1e-8, g_tol=1e-8, iterations=1000, delta=None,
                      lower=(), upper=(), ctx=None, full_trace=False, loss="linear", f_scale=1.0, sigma=None):
    """B runs of optimize! in one device loop: nls.J is a BlockDiagonal(B, mb, nb) and fit b is the problem made of residual
    rows b*mb .. and parameters b*nb .. -- its own trust region, accept decisions, convergence test and counts
    (levenberg_marquardt.jl:39-144 / dogleg.jl:41-203 per block; include/lsqhip.h: lsq_optimize_batched).  f_ / g_ have the
    signatures optimize_ uses and see the stacked x, y, J.data; they must be block-separable and deterministic.  Default
    optimizer: LevenbergMarquardt(Cholesky()).  A fit that fails (status[b] != 0) does not end the call.  Mutates nls.x,
    nls.y, nls.J; returns a BatchedResult.  loss, f_scale, sigma: as for optimize_ (sigma has m entries; the result's
    `outliers` counts all blocks)."""
    n, m = len(nls.x), len(nls.y)
    optimizer, solver = _batched_arguments(nls.J, optimizer, n, lower, upper)
    if loss != "linear" or sigma is not None:
        loss, f_scale, sigma = _loss_arguments(loss, f_scale, sigma, m)      # (refusals before anything is allocated)
    ctx = ctx or default_context()
    J = nls.J
    Jd = DeviceMatrix(ctx, J)
    dx, dy = DeviceVector(ctx, n, nls.x), DeviceVector(ctx, m, nls.y)
    host = _HostCallbacks(ctx, nls, Jd)
    F, G, user = host.F, host.G, None
    lossobj = _new_loss(ctx, loss, f_scale, sigma, m)
    if lossobj is not None:
        lossobj.set_problem(host.F, None if host.device_fd else host.G)
        F, user = lossobj.F, lossobj.h
        G = host.G if host.device_fd else lossobj.G
    st = r = None
    try:
        host.bind()
        st, r = _run_native_batched(ctx, optimizer.kind, solver.kind, Jd.h, (J.nblocks, J.mb, J.nb), dx, dy, F, G,
                                    user, x_tol, f_tol, g_tol, iterations, delta, lower, upper, full_trace, optimizer.name)
    finally:
        host.release()
        if st is not None:
            host.fetch_jacobian()
            if lossobj is not None:
                host.fetch_scaled_jacobian()
            nls.x[:] = dx.get()
            nls.y[:] = dy.get()
    try:
        if host.err:
            raise host.err[0]
        check(st)
        if lossobj is not None:
            r.loss, r.f_scale, r.outliers = lossobj.loss, lossobj.f_scale, _loss_outliers(lossobj, host, dx)
    finally:
        if lossobj is not None:
            lossobj.free()
    r.minimizer = nls.x
    r.jacobian = nls.J
    Jd.free()
    return r


class LeastSquaresProblemAllocated:
    """LeastSquaresProblemAllocated(nls, optimizer) (types.jl:141-160, exported by the reference): the problem
    together with its optimizer, its solver and every buffer they need, allocated once; `optimize_(nlsa)` can then
    be called repeatedly (e.g. from different starting points written into `nlsa.x`) without allocating -- the
    device Jacobian handle, the vectors and, inside the library, the loop/solver workspace are all reused.
    loss, f_scale, sigma: the robust loss and the observation weights of optimize_, taken here."""

    def __init__(self, nls, optimizer=None, ctx=None, loss="linear", f_scale=1.0, sigma=None):
        if not isinstance(nls, LeastSquaresProblem):
            raise TypeError("LeastSquaresProblemAllocated(nls::LeastSquaresProblem, optimizer)")
        self.ctx = ctx or default_context()
        self.solver = default_solver(optimizer.solver if optimizer is not None else None, nls.J)
        self.optimizer = default_optimizer(optimizer, self.solver, nls.J)
        self.x, self.y, self.f_, self.J, self.g_ = nls.x, nls.y, nls.f_, nls.J, nls.g_
        self._fd_g = getattr(nls, "_fd_g", None)     # (g_ left to the default on a block handle: central differences on the device)
        self._fd_colouring = getattr(nls, "_fd_colouring", None)   # (or to "central_coloured" on a sparse one)
        self._Jd = nls.J if isinstance(nls.J, DeviceOperator) else DeviceMatrix(self.ctx, nls.J)
        self._dx = DeviceVector(self.ctx, len(nls.x), nls.x)
        self._dy = DeviceVector(self.ctx, len(nls.y), nls.y)
        # the page-locked staging buffer of the Jacobian uploads is part of the allocated problem too
        self._stage = None if isinstance(self._Jd, DeviceOperator) else PinnedBuffer(self.ctx, self._Jd.nnz)
        # ... and so is the loss object (loss, f_scale, sigma are taken here: optimize_ allocates nothing)
        self._loss = _new_loss(self.ctx, loss, f_scale, sigma, len(nls.y))

    def free(self):
        if getattr(self, "_loss", None) is not None:
            self._loss.free()
            self._loss = None
        if self._Jd is not None and not isinstance(self._Jd, DeviceOperator):
            self._Jd.free()
        self._Jd = None
        if getattr(self, "_stage", None) is not None:
            self._stage.free()
            self._stage = None


def optimize(f, x, optimizer, autodiff="central", J=None, colouring=None, **kwargs):
    """optimize(f, x, optimizer; kwargs...) -- types.jl:182-184 (x is copied; f returns a vector).
    autodiff="central_coloured" with J = a scipy.sparse pattern (and optionally a colouring): coloured central differences on
    the device, as LeastSquaresProblem describes.  loss=, f_scale= and sigma= go to optimize_ with the other keywords."""
    x0 = np.array(x, dtype=np.float64)
    out0 = np.atleast_1d(np.asarray(f(x0), dtype=np.float64))

    def f_(out, xx):
        out[:] = np.atleast_1d(f(xx))

    nls = LeastSquaresProblem(x=x0.copy(), f_=f_, J=J, output_length=len(out0), autodiff=autodiff, colouring=colouring)
    return optimize_(nls, optimizer, **kwargs)
