"""BlockQR() without a GPU: the selector, the refusals that are decided in Python, the declaration of the new entry point."""
import os

import numpy as np
import pytest

import lsq_amd as lsq


def test_blockqr_is_a_solver_kind_of_its_own():
    assert lsq.BlockQR.kind == lsq._lib.BLOCK_QR == 3
    assert (lsq._lib.QR, lsq._lib.CHOLESKY, lsq._lib.LSMR) == (0, 1, 2)            # the existing values do not move
    assert issubclass(lsq.BlockQR, lsq.api.AbstractSolver) and "BlockQR" in lsq.__all__


def test_default_solver_and_optimizer():
    J = lsq.BlockDiagonal(3, 4, 2)
    s = lsq.default_solver(lsq.BlockQR(), J)
    assert isinstance(s, lsq.BlockQR)
    assert isinstance(lsq.default_optimizer(None, s), lsq.Dogleg)                 # as for QR()
    assert isinstance(lsq.default_optimizer(lsq.LevenbergMarquardt(), s), lsq.LevenbergMarquardt)
    assert isinstance(lsq.default_optimizer(lsq.Dogleg(), s), lsq.Dogleg)
    assert isinstance(lsq.default_solver(lsq.BlockQR(), lsq.BlockDiagonal(1, 3, 64)), lsq.BlockQR)    # wide blocks are fine
    # what was there stays
    assert isinstance(lsq.default_solver(None, J), lsq.LSMR)
    assert isinstance(lsq.default_solver(None, np.zeros((4, 2))), lsq.QR)
    assert isinstance(lsq.LevenbergMarquardt(lsq.BlockQR).solver, lsq.BlockQR)     # a class is instantiated


def test_sparse_matrices_are_refused():
    sp = pytest.importorskip("scipy.sparse")
    J = lsq.BlockDiagonal(3, 4, 2)
    for other in (J.tocsc(), sp.identity(6, format="csc")):       # the same pattern as a plain CSC matrix: no pattern sniffing
        with pytest.raises(lsq.ArgumentError) as e:
            lsq.default_solver(lsq.BlockQR(), other)
        assert e.value.status == lsq._lib.EARG and "BlockDiagonal" in str(e.value)


def test_refusals_decided_in_python():
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.default_solver(lsq.BlockQR(), np.zeros((12, 6)))
    assert e.value.status == lsq._lib.EARG and "BlockDiagonal" in str(e.value)
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.default_solver(lsq.BlockQR(), lsq.BlockDiagonal(2, 70, 65))
    assert e.value.status == lsq._lib.EARG and "64" in str(e.value) and "70 x 65" in str(e.value)
    f_ = lambda out, x: None
    g_ = lambda J, x: None
    with pytest.raises(lsq.ArgumentError) as e:       # optimize_ refuses before it touches a device
        lsq.optimize_(lsq.LeastSquaresProblem(x=np.zeros(6), f_=f_, g_=g_, J=np.zeros((12, 6))), lsq.Dogleg(lsq.BlockQR()))
    assert e.value.status == lsq._lib.EARG
    wide = lsq.BlockDiagonal(2, 70, 65)
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.optimize_batched_(lsq.LeastSquaresProblem(x=np.zeros(130), f_=f_, g_=g_, J=wide), lsq.Dogleg(lsq.BlockQR()))
    assert e.value.status == lsq._lib.EARG and "70 x 65" in str(e.value)


def test_qr_on_a_block_diagonal_keeps_its_old_text():
    J = lsq.BlockDiagonal(3, 4, 2)
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.default_solver(lsq.QR(), J)
    assert str(e.value) == "solver QR() is not available for sparse Jacobians. Choose between Cholesky() and LSMR()"
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.optimize_batched_(lsq.LeastSquaresProblem(x=np.zeros(6), f_=lambda o, x: None, g_=lambda J, x: None, J=J),
                              lsq.Dogleg(lsq.QR()))
    assert str(e.value) == "solver QR() is not available for sparse Jacobians. Choose between Cholesky() and LSMR()"


def test_new_entry_point_declared():
    assert "lsq_solver_blockdiag_ranks" in lsq.declared_symbols()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "lsqhip.h")).read()
    assert "int lsq_solver_blockdiag_ranks(const lsq_solver *s, int *h_ranks);" in header
    assert "LSQ_QR = 0, LSQ_CHOLESKY = 1, LSQ_LSMR = 2, LSQ_BLOCK_QR = 3" in header


def test_batched_inner_counts_one_solve():
    r = lsq.BatchedResult(2, 3, 2, optimizer="Dogleg")
    r.iterations[:] = 3
    r.trace = dict(ssr=np.zeros((3, 2)), gnorm=np.zeros((3, 2)), delta=np.zeros((3, 2)), rho=np.zeros((3, 2)),
                   accept=np.array([[1, 0], [0, 1], [1, 1]], dtype=np.int32), x=np.zeros((3, 4)))
    assert list(r.block(0).trace["inner"]) == [1, 1, 0] and list(r.block(1).trace["inner"]) == [1, 0, 1]
