"""BorderedQR() on bordered block-diagonal Jacobians, host tier (no device): the numpy twin of lsq_borderedqr.hip's stages
against the fp64 Householder solve of the stacked matrix on every shape the device tests use; the certification of the accuracy
case list -- the twin passes the tier's rule (accuracy_common.judge against the longdouble Householder solve, e_ref from the
fp64 Householder solve) on every case tests/test_u_gpu_borderedqr.py runs on the device, and the fp64 NORMAL equations are
beyond that bound on every `ill6` case, so the cases tell a backward-stable solver from one that squares the condition number;
the expected LSQ_ERANK columns; the BorderedQR() rules of default_solver / default_optimizer with every refusal text."""
import os
import re

import numpy as np
import pytest

import accuracy_common as ac
import borderedqr_common as bq
import lsq_amd as lsq
import schur_common as sc


# ------------------------------------------------------------------------------------------ 1. the twin is the solve
@pytest.mark.parametrize("B,mb,nb,ng", sc.SOLVE_SHAPES)
def test_twin_against_the_fp64_householder_solve(B, mb, nb, ng):
    J, y, damp = sc.solve_operand(B, mb, nb, ng)
    x, col = bq.twin_solve(J, y, damp)
    assert col == 0
    err = sc.rel_err(x, bq.qr_fp64_solve_any(J, y, damp))
    print("twin B=%d mb=%d nb=%d ng=%d rel err %.3e" % (B, mb, nb, ng, err))
    assert err <= sc.SOLVE_RTOL


def test_blockwise_reference_is_the_dense_one():
    J, y, damp = sc.solve_operand(7, 20, 5, 70)
    assert J.shape[1] <= bq.DENSE_QR_MAX_N
    old = bq.DENSE_QR_MAX_N
    try:
        bq.DENSE_QR_MAX_N = 0
        xb = bq.qr_fp64_solve_any(J, y, damp)
    finally:
        bq.DENSE_QR_MAX_N = old
    assert sc.rel_err(xb, bq.qr_fp64_reference(J, y, damp)) <= 1e-12


def test_twin_column_scaled():
    B, mb, nb, ng = 7, 20, 5, 70
    V, y, damp = sc.solve_operand(B, mb, nb, ng)
    s = 0.25 + np.random.default_rng(3).random(B * nb + ng)
    J = lsq.BorderedBlockDiagonal(B, mb, nb, ng, data=ac.bb_scale_values(V, s))
    x, col = bq.twin_solve(V, y, damp, colscale=s)
    assert col == 0 and sc.rel_err(x, bq.qr_fp64_reference(J, y, damp)) <= sc.SOLVE_RTOL


# ------------------------------------------------------------------------------------------ 2. the accuracy cases are certified
@pytest.mark.parametrize("family,shape", sc.acc_cases())
def test_twin_passes_the_accuracy_rule(family, shape):
    B, mb, nb, ng = shape
    for zero in ((False, True) if family == "ill" else (False,)):
        op, damp, ref = bq.acc_reference(family, shape, zero)
        x, col = bq.twin_solve(op.J, op.y, damp)
        assert col == 0
        ac.judge("bordered-qr twin %s B=%d nb=%d ng=%d%s" % (family, B, nb, ng, " zero damping" if zero else ""), ref.pieces(x))
    if family == "graded":
        op, damp, ref = bq.acc_reference(family, shape, False, True)
        x, col = bq.twin_solve(op.V, op.y, damp, colscale=op.s)
        assert col == 0
        ac.judge("bordered-qr twin %s B=%d nb=%d ng=%d colscale" % (family, B, nb, ng), ref.pieces(x))


@pytest.mark.parametrize("shape", bq.ILL6_SHAPES)
def test_ill6_tells_the_two_kinds_of_solver_apart(shape):
    """The twin is inside the bound under both right-hand sides, the fp64 normal equations are beyond it under both."""
    B, mb, nb, ng = shape
    assert mb >= nb + ng
    ops, ref = bq.ill6_reference(shape)
    for col, rhs in enumerate(ac.RHS):
        op = ops[rhs]
        x, bad = bq.twin_solve(op.J, op.y, op.damp)
        assert bad == 0
        ac.judge("bordered-qr twin ill6 B=%d nb=%d ng=%d %s" % (B, nb, ng, rhs), ref.pieces(x, col))
        over = bq.beyond(ref.pieces(ac.bb_fp64_solve(op.J, op.y, op.damp), col))
        print("   fp64 normal equations: %.1f x the bound" % over)
        assert over > 1.0, (shape, rhs, over)


# ------------------------------------------------------------------------------------------ 3. LSQ_ERANK
def test_rank_cases_name_the_lowest_stacked_column():
    for name, expect in (("zero", 8), ("two", 6), ("nan", 4)):
        J, y, damp, col = bq.rank_case(name)
        assert col == expect
        assert bq.twin_solve(J, y, damp) == (None, expect)
    for name in ("damped", "good"):
        J, y, damp, col = bq.rank_case(name)
        x, bad = bq.twin_solve(J, y, damp)
        assert (col, bad) == (0, 0) and sc.rel_err(x, bq.qr_fp64_reference(J, y, damp)) <= sc.SOLVE_RTOL


# ------------------------------------------------------------------------------------------ 4. the rules
def _problem(J):
    return lsq.LeastSquaresProblem(x=np.zeros(J.shape[1]), f_=lambda o, x: None, g_=lambda J, x: None, J=J)


def test_bordered_qr_rules():
    assert lsq.BorderedQR.kind == lsq._lib.BORDERED_QR == 5
    J = lsq.BorderedBlockDiagonal(3, 80, 2, 70)
    s = lsq.default_solver(lsq.BorderedQR(), J)
    assert isinstance(s, lsq.BorderedQR)
    assert isinstance(lsq.default_solver(lsq.BorderedQR(), lsq.BorderedBlockDiagonal(3, 1, 64, 1000)), lsq.BorderedQR)
    assert isinstance(lsq.default_solver(lsq.BorderedQR(), lsq.BorderedBlockDiagonal(3, 4, 2, 2)), lsq.BorderedQR)
    assert isinstance(lsq.default_solver(None, J), lsq.LSMR)                    # the default does not change
    o = lsq.default_optimizer(None, s, J)
    assert isinstance(o, lsq.LevenbergMarquardt) and o.solver is s
    assert isinstance(lsq.default_optimizer(lsq.LevenbergMarquardt(), s, J), lsq.LevenbergMarquardt)
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.default_optimizer(lsq.Dogleg(), s, J)
    assert e.value.status == lsq._lib.EARG and str(e.value) == lsq.api.BORDERED_DOGLEG_TEXT
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.optimize_(_problem(J), lsq.Dogleg(lsq.BorderedQR()))
    assert str(e.value) == lsq.api.BORDERED_DOGLEG_TEXT


def test_bordered_qr_refusal_texts():
    for J, name in ((np.zeros((6, 3)), "ndarray"), (lsq.BlockDiagonal(3, 4, 2), "BlockDiagonal")):
        with pytest.raises(lsq.ArgumentError) as e:
            lsq.default_solver(lsq.BorderedQR(), J)
        assert e.value.status == lsq._lib.EARG
        assert str(e.value) == lsq.api.BORDERED_QR_HANDLE_TEXT % (name, tuple(J.shape))
        assert "BorderedQR() needs a BorderedBlockDiagonal" in str(e.value) and "LSMR()" in str(e.value) and "BlockQR()" in str(e.value)
    sp = pytest.importorskip("scipy.sparse")
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.default_solver(lsq.BorderedQR(), sp.eye(5, format="csc"))
    assert "BorderedQR() needs a BorderedBlockDiagonal" in str(e.value)
    K = lsq.BorderedBlockDiagonal(2, 70, 65, 5)
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.default_solver(lsq.BorderedQR(), K)
    assert str(e.value) == lsq.api.BORDERED_QR_NB_TEXT % (65, 5) and "nb <= 64" in str(e.value) and "LSMR()" in str(e.value)
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.optimize_(_problem(K), lsq.LevenbergMarquardt(lsq.BorderedQR()))
    assert "nb <= 64" in str(e.value)
    # optimize_batched_: the container is refused first on a bordered Jacobian, the solver on a block-diagonal one
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.optimize_batched_(_problem(lsq.BorderedBlockDiagonal(3, 4, 2, 70)), lsq.LevenbergMarquardt(lsq.BorderedQR()))
    assert "BorderedBlockDiagonal" in str(e.value) and "optimize_" in str(e.value)
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.optimize_batched_(_problem(lsq.BlockDiagonal(3, 4, 2)), lsq.LevenbergMarquardt(lsq.BorderedQR()))
    assert "BorderedQR()" in str(e.value) and "LevenbergMarquardt(BorderedQR())" in str(e.value)


def test_kind_is_declared_in_the_header_and_the_shim():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "lsqhip.h")).read()
    assert re.search(r"enum \{ LSQ_BORDERED_QR = 5 \};", text)
    assert "const LSQ_BORDERED_QR = 5" in open(os.path.join(root, "INTEGRATION.md")).read()
