"""Schur() on bordered block-diagonal Jacobians, host tier (no device): the numpy twin of lsq_schur.hip's five steps against the
fp64 reference and a dense unpivoted Cholesky of the stacked normal matrix on every shape the device tests use, the Schur()
rules of default_solver / default_optimizer (and that every other solver's rules answer what they did), the refusal texts,
the expected PosDefException columns, and the certification of the accuracy case list: the twin passes the tier's rule
(accuracy_common.judge, factor 16, longdouble reference) on every case tests/test_r_gpu_schur.py runs on the device."""
import os
import re

import numpy as np
import pytest

import accuracy_common as ac
import lsq_amd as lsq
import schur_common as sc


# ------------------------------------------------------------------------------------------ 1. the case list covers what it claims
def test_branch_shapes_cover_every_size_twice():
    sizes = (sc.BS, sc.MBS, sc.NBS, sc.NGS)
    for d, values in enumerate(sizes):
        assert {c[d] for c in sc.BRANCH_SHAPES} == set(values)
        for v in values:
            rows = [c for c in sc.BRANCH_SHAPES if c[d] == v]
            for e in range(4):
                if e != d:
                    assert len({r[e] for r in rows}) >= 2, (d, v, e)
    assert any(mb < nb for _, mb, nb, _ in sc.BRANCH_SHAPES)
    assert sum(nb + ng > 64 for _, _, nb, ng in sc.ACC_SHAPES) >= 3 and len(sc.ACC_SHAPES) >= 6
    assert all(B * nb + ng <= 400 and mb >= nb + ng for B, mb, nb, ng in sc.ACC_SHAPES)
    assert all(nb + ng <= 64 for nb, ng in sc.AGREE_SHAPES)


# ------------------------------------------------------------------------------------------ 2. the twin is the solve
@pytest.mark.parametrize("B,mb,nb,ng", sc.SOLVE_SHAPES)
def test_twin_against_fp64_reference_and_stacked_cholesky(B, mb, nb, ng):
    J, y, damp = sc.solve_operand(B, mb, nb, ng)
    x, col = sc.twin_solve(J, y, damp)
    assert col == 0
    assert sc.rel_err(x, ac.bb_fp64_solve(J, y, damp)) <= sc.SOLVE_RTOL
    if J.shape[1] <= 700:
        D = J.toarray()
        U, bad = sc.chol_upper(D.T @ D + np.diag(damp))
        assert bad == 0
        xs = sc.backward(U, sc.forward(U, D.T @ y))
        assert sc.rel_err(x, xs) <= sc.SOLVE_RTOL


def test_twin_column_scaled():
    B, mb, nb, ng = 7, 20, 5, 70
    V, y, damp = sc.solve_operand(B, mb, nb, ng)
    s = 0.25 + np.random.default_rng(3).random(B * nb + ng)
    J = lsq.BorderedBlockDiagonal(B, mb, nb, ng, data=ac.bb_scale_values(V, s))
    x, col = sc.twin_solve(V, y, damp, colscale=s)
    assert col == 0 and sc.rel_err(x, ac.bb_fp64_solve(J, y, damp)) <= sc.SOLVE_RTOL


# ------------------------------------------------------------------------------------------ 3. the failure cases
EXPECTED_COLUMNS = {"local": 4, "border": 8, "twin": 9, "both": 5, "border blocked": 3 * 17 + 38, "twin blocked": 3 * 5 + 67,
                    "both blocked": 17 + 17}


@pytest.mark.parametrize("name", sorted(sc.FAILURES))
def test_failure_columns_are_the_stacked_cholesky_columns(name):
    J, y, damp = sc.failure_case(name)
    assert np.all(J.data == np.round(J.data)) and np.all(y == np.round(y))
    col = sc.stacked_potrf_column(J, damp)
    assert col == EXPECTED_COLUMNS[name]
    assert sc.twin_solve(J, y, damp) == (None, col)
    # ... and the same operand without its defect is positive definite, with S = 4 I
    B, nb, ng, rows, _ = sc.FAILURES[name]
    K, yk, dk = sc.exact_operand(B, nb, ng, rows)
    assert sc.stacked_potrf_column(K, dk) == 0
    x, c0 = sc.twin_solve(K, yk, dk)
    assert c0 == 0 and sc.rel_err(x, ac.bb_fp64_solve(K, yk, dk)) <= sc.SOLVE_RTOL


# ------------------------------------------------------------------------------------------ 4. the accuracy cases are certified
@pytest.mark.parametrize("family,shape", sc.acc_cases())
def test_twin_passes_the_accuracy_rule(family, shape):
    B, mb, nb, ng = shape
    op = ac.bb_operand(family, B, mb, nb, ng, sc.acc_seed(B, nb, ng))
    damps = [("", op.damp)] + ([(" zero damping", np.zeros(B * nb + ng))] if family == "ill" else [])
    for dlabel, damp in damps:
        x, col = sc.twin_solve(op.J, op.y, damp)
        assert col == 0
        ac.judge("schur twin %s B=%d nb=%d ng=%d%s" % (family, B, nb, ng, dlabel), ac.bb_solve_pieces(op, x, damp))
    if op.V is not None:
        x, col = sc.twin_solve(op.V, op.y, op.damp, colscale=op.s)
        assert col == 0
        ac.judge("schur twin %s B=%d nb=%d ng=%d colscale" % (family, B, nb, ng), ac.bb_solve_pieces(op, x, op.damp, True))


# ------------------------------------------------------------------------------------------ 5. the rules
def _problem(J):
    return lsq.LeastSquaresProblem(x=np.zeros(J.shape[1]), f_=lambda o, x: None, g_=lambda J, x: None, J=J)


def test_schur_rules():
    assert lsq.Schur.kind == lsq._lib.SCHUR == 4
    J = lsq.BorderedBlockDiagonal(3, 80, 2, 70)
    s = lsq.default_solver(lsq.Schur(), J)
    assert isinstance(s, lsq.Schur)
    assert isinstance(lsq.default_solver(lsq.Schur(), lsq.BorderedBlockDiagonal(3, 4, 64, 1000)), lsq.Schur)
    assert isinstance(lsq.default_solver(lsq.Schur(), lsq.BorderedBlockDiagonal(3, 4, 2, 2)), lsq.Schur)     # nb + ng <= 64 too
    o = lsq.default_optimizer(None, s, J)
    assert isinstance(o, lsq.LevenbergMarquardt) and o.solver is s
    assert isinstance(lsq.default_optimizer(lsq.LevenbergMarquardt(), s, J), lsq.LevenbergMarquardt)
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.default_optimizer(lsq.Dogleg(), s, J)
    assert e.value.status == lsq._lib.EARG and str(e.value) == lsq.api.BORDERED_DOGLEG_TEXT
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.optimize_(_problem(J), lsq.Dogleg(lsq.Schur()))
    assert str(e.value) == lsq.api.BORDERED_DOGLEG_TEXT


def test_schur_refusal_texts():
    for J, name in ((np.zeros((6, 3)), "ndarray"), (lsq.BlockDiagonal(3, 4, 2), "BlockDiagonal")):
        with pytest.raises(lsq.ArgumentError) as e:
            lsq.default_solver(lsq.Schur(), J)
        assert e.value.status == lsq._lib.EARG
        assert str(e.value) == lsq.api.SCHUR_HANDLE_TEXT % (name, tuple(J.shape))
        assert "Schur() needs a BorderedBlockDiagonal" in str(e.value) and "LSMR()" in str(e.value) and "Cholesky()" in str(e.value)
    sp = pytest.importorskip("scipy.sparse")
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.default_solver(lsq.Schur(), sp.eye(5, format="csc"))
    assert "Schur() needs a BorderedBlockDiagonal" in str(e.value)
    K = lsq.BorderedBlockDiagonal(2, 70, 65, 5)
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.default_solver(lsq.Schur(), K)
    assert str(e.value) == lsq.api.SCHUR_NB_TEXT % (65, 5) and "nb <= 64" in str(e.value) and "LSMR()" in str(e.value)
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.optimize_(_problem(K), lsq.LevenbergMarquardt(lsq.Schur()))
    assert "nb <= 64" in str(e.value)
    # optimize_batched_: the container is refused first on a bordered Jacobian, the solver on a block-diagonal one
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.optimize_batched_(_problem(lsq.BorderedBlockDiagonal(3, 4, 2, 70)), lsq.LevenbergMarquardt(lsq.Schur()))
    assert "BorderedBlockDiagonal" in str(e.value) and "optimize_" in str(e.value)
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.optimize_batched_(_problem(lsq.BlockDiagonal(3, 4, 2)), lsq.LevenbergMarquardt(lsq.Schur()))
    assert "Schur()" in str(e.value) and "LevenbergMarquardt(Schur())" in str(e.value)


def test_rules_of_every_other_solver_are_what_they_were():
    B_ = lsq.BorderedBlockDiagonal(3, 4, 2, 2)
    D_ = lsq.BlockDiagonal(3, 4, 2)
    M_ = np.zeros((6, 3))
    assert isinstance(lsq.default_solver(None, B_), lsq.LSMR) and isinstance(lsq.default_solver(None, D_), lsq.LSMR)
    assert isinstance(lsq.default_solver(None, M_), lsq.QR)
    for J in (B_, D_, M_):
        for S in (lsq.Cholesky, lsq.LSMR):
            s = S()
            assert lsq.default_solver(s, J) is s
    assert isinstance(lsq.default_solver(lsq.QR(), M_), lsq.QR) and isinstance(lsq.default_solver(lsq.BlockQR(), D_), lsq.BlockQR)
    for J, S in ((B_, lsq.QR), (B_, lsq.BlockQR), (D_, lsq.QR), (M_, lsq.BlockQR)):
        with pytest.raises(lsq.ArgumentError):
            lsq.default_solver(S(), J)
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.default_solver(lsq.Cholesky(), lsq.BorderedBlockDiagonal(2, 70, 60, 5))
    assert "nb + ng <= 64" in str(e.value) and "Use LSMR()" in str(e.value)
    c = lsq.Cholesky()
    assert isinstance(lsq.default_optimizer(None, c), lsq.Dogleg) and isinstance(lsq.default_optimizer(None, c, D_), lsq.Dogleg)
    assert isinstance(lsq.default_optimizer(None, c, B_), lsq.LevenbergMarquardt)
    assert isinstance(lsq.default_optimizer(None, lsq.LSMR(), B_), lsq.LevenbergMarquardt)
    assert isinstance(lsq.default_optimizer(lsq.Dogleg(), lsq.LSMR(), B_), lsq.Dogleg)
    assert isinstance(lsq.default_optimizer(None, lsq.QR()), lsq.Dogleg)
    assert isinstance(lsq.default_optimizer(lsq.LevenbergMarquardt(), lsq.QR()), lsq.LevenbergMarquardt)
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.default_optimizer(lsq.Dogleg(), c, B_)
    assert str(e.value) == lsq.api.BORDERED_DOGLEG_TEXT


def test_kind_is_declared_in_the_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "lsqhip.h")).read()
    m = re.search(r"typedef enum \{([^}]*)\} lsq_solver_kind;", text)
    kinds = dict((k.strip(), int(v)) for k, v in (item.split("=") for item in m.group(1).split(",")))
    assert kinds == {"LSQ_QR": 0, "LSQ_CHOLESKY": 1, "LSQ_LSMR": 2, "LSQ_BLOCK_QR": 3, "LSQ_SCHUR": 4}
    assert (lsq._lib.QR, lsq._lib.CHOLESKY, lsq._lib.LSMR, lsq._lib.BLOCK_QR, lsq._lib.SCHUR) == (0, 1, 2, 3, 4)
