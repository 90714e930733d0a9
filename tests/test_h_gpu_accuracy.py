"""Accuracy tier on the device: the Cholesky block solvers (lsq_blockdiag.hip, lsq_bordered.hip), the covariance kernels
(lsq_cov.hip, k_bb_cov_*), the dense Cholesky paths, the CholeskyQR2 panel and BlockQR() are held to LAPACK's OWN error.

The shape tier (test_b, test_c, test_e, test_f, test_g) compares with fp64 numpy at rel 1e-9, normwise over a whole vector or
block, on operands whose Gram matrices have condition numbers below 10: six to seven digits could be lost unnoticed.  Here the
reference is numpy.longdouble (tests/hp_reference.py), the error is measured per piece in a scaling-invariant metric, and the
device must satisfy

    e_dev <= 16 * max(e_ref, min(max(16, k), 64) * 2^-53)

where e_ref is the error of fp64 numpy / LAPACK on the same operand (tests/accuracy_common.py has the metrics, the rule and
the operand families plain / graded / ill / far; tests/test_accuracy_host.py shows on the CPU that the rule passes an fp64
stand-in of the device algorithm and rejects one whose reciprocal square root is only good to 2^-24).  Every case prints the
piece closest to its bound: e_dev, e_ref, their ratio."""
import numpy as np
import pytest

import accuracy_common as ac
import hp_reference as hp
from gpu_common import lsq
from test_e_gpu_blockqr import bq_solve, oracle_blocks

pytestmark = pytest.mark.gpu

MB_BORDERED = 96


def solve(ctx, Jd, y, damp, solver=None, for_lm=None):
    sv = lsq.AllocatedSolver(Jd, solver or lsq.Cholesky(), for_lm=(damp is not None) if for_lm is None else for_lm)
    dx = lsq.DeviceVector(ctx, Jd.n)
    dd = lsq.DeviceVector(ctx, Jd.n, damp) if damp is not None else None
    sv.ldiv_(dx, lsq.DeviceVector(ctx, Jd.m, y), dd)
    return dx.get(), sv


def handles(ctx, op):
    """(label, handle, scaled_handle): the operand multiplied out, and -- graded -- the same operand as V with the grading in s."""
    out = [("", lsq.DeviceMatrix(ctx, op.J), False)]
    if op.V is not None:
        Jd = lsq.DeviceMatrix(ctx, op.V)
        Jd.set_colscale(lsq.DeviceVector(ctx, Jd.n, op.s))
        out.append((" colscale", Jd, True))
    return out


# ------------------------------------------------------------------------------------------ 1. block-diagonal Cholesky(), damped
@pytest.mark.parametrize("family", ac.FAMILIES)
@pytest.mark.parametrize("nb", ac.BD_NBS)
def test_blockdiag_damped(ctx, nb, family):
    """k_bd_solve<1|4, false>: one wavefront per block (5, 16) and one workgroup per block with 2, 3, 4 tile rows."""
    op = ac.bd_operand(family, ac.BD_B, ac.BD_MB, nb, ac.bd_seed(nb))
    for label, Jd, scaled in handles(ctx, op):
        x, sv = solve(ctx, Jd, op.y, op.damp)
        info = sv.info()
        assert info["blockdiag_path"] == "batched-unpivoted" and info["blockdiag_block"] == -1
        ac.judge("blockdiag damped %s nb=%d%s" % (family, nb, label), ac.bd_solve_pieces(op, x, op.damp, scaled))


# ------------------------------------------------------------------------------------------ 2. block-diagonal Cholesky(), pivoted
@pytest.mark.parametrize("family", ["plain", "graded", "ill"])
@pytest.mark.parametrize("nb", ac.BD_NBS)
def test_blockdiag_undamped_pivoted(ctx, nb, family):
    """k_bd_solve<., true>; every block has full rank: nothing may be reported deficient."""
    op = ac.bd_operand(family, ac.BD_B, ac.BD_MB, nb, ac.bd_seed(nb))
    for label, Jd, scaled in handles(ctx, op):
        x, sv = solve(ctx, Jd, op.y, None)
        info = sv.info()
        assert info["blockdiag_path"] == "batched-pivoted" and info["blockdiag_block"] == -1
        ac.judge("blockdiag pivoted %s nb=%d%s" % (family, nb, label), ac.bd_solve_pieces(op, x, None, scaled))


# ------------------------------------------------------------------------------------------ 3. bordered Schur
BB_SOLVE_SHAPES = [(5, 3), (15, 1), (16, 17), (40, 24), (1, 63), (63, 1)]


@pytest.mark.parametrize("family", ac.FAMILIES)
@pytest.mark.parametrize("B", [5, 70])
@pytest.mark.parametrize("nb,ng", BB_SOLVE_SHAPES)
def test_bordered_schur(ctx, nb, ng, B, family):
    """k_bb_eliminate, k_bb_reduce (B = 70: the contributions are summed in groups of 64), k_bb_schur, k_bb_back.  Pieces: every
    block and the shared part.  ill also with zero damping (the bordered solver has no undamped entry point)."""
    op = ac.bb_operand(family, B, MB_BORDERED, nb, ng, 1000 * nb + 10 * ng + B)
    damps = [("", op.damp)] + ([(" zero damping", np.zeros(B * nb + ng))] if family == "ill" else [])
    for label, Jd, scaled in handles(ctx, op):
        for dlabel, damp in damps:
            x, sv = solve(ctx, Jd, op.y, damp)
            info = sv.info()
            assert info["blockdiag_path"] == "bordered-schur" and info["blockdiag_block"] == -1
            ac.judge("bordered %s nb=%d ng=%d B=%d%s%s" % (family, nb, ng, B, label, dlabel), ac.bb_solve_pieces(op, x, damp, scaled))


# ------------------------------------------------------------------------------------------ 4. covariance, block-diagonal
@pytest.mark.parametrize("family", ["plain", "graded", "ill"])
@pytest.mark.parametrize("nb", ac.BD_NBS)
def test_covariance_blockdiag(ctx, nb, family):
    B, mb = ac.BD_B, ac.BD_MB
    op = ac.bd_operand(family, B, mb, nb, ac.bd_seed(nb) + 1)
    f = np.random.default_rng(nb).standard_normal(B * mb)
    for label, Jd, scaled in handles(ctx, op):
        sv = lsq.AllocatedSolver(Jd, lsq.Cholesky(), for_lm=True)
        H0 = [hp.inv_gram(ac.bd_effective(op, b, scaled)) for b in range(B)]
        R0 = [np.linalg.inv(op.J.block(b).T @ op.J.block(b)) for b in range(B)]
        for flabel, ff in ((" no f", None), (" with f", f)):
            cov = sv.covariance(f=ff)
            assert np.array_equal(cov.info, np.zeros(B, dtype=np.int32))
            pieces = []
            for b in range(B):
                fb = f[b * mb:(b + 1) * mb]
                H = H0[b] if ff is None else H0[b] * ac.s2_of(fb, mb - nb)
                Cref = R0[b] if ff is None else np.sum(fb ** 2) / (mb - nb) * R0[b]
                pieces += ac.cov_pieces("block %d" % b, cov.block(b), cov.stderr[b * nb:(b + 1) * nb], Cref, H, nb)
            ac.judge("covariance blockdiag %s nb=%d%s%s" % (family, nb, label, flabel), pieces)


# ------------------------------------------------------------------------------------------ 5. covariance, bordered
BB_COV_SHAPES = [(3, 2), (16, 1), (20, 12), (40, 24), (1, 63), (63, 1)]


@pytest.mark.parametrize("family", ["plain", "graded", "ill"])
@pytest.mark.parametrize("B", [5, 70])
@pytest.mark.parametrize("nb,ng", BB_COV_SHAPES)
def test_covariance_bordered(ctx, nb, ng, B, family):
    """k_bb_cov_schur / k_bb_cov_back behind the elimination; e_ref: numpy.linalg.inv of the dense J'J, as
    test_g_gpu_covariance.py forms it."""
    mb = MB_BORDERED
    op = ac.bb_operand(family, B, mb, nb, ng, 2000 * nb + 10 * ng + B)
    m, n = B * mb, B * nb + ng
    f = np.random.default_rng(nb + ng + B).standard_normal(m)
    D = op.J.toarray()
    R0 = np.linalg.inv(D.T @ D)
    for label, Jd, scaled in handles(ctx, op):
        sv = lsq.AllocatedSolver(Jd, lsq.Cholesky(), for_lm=True)
        loc, shared = hp.inv_gram(op.V, colscale=op.s) if scaled else hp.inv_gram(op.J)
        for flabel, ff in ((" no f", None), (" with f", f)):
            cov = sv.covariance(f=ff)
            assert cov.info is None and sv.info()["blockdiag_block"] == -1
            s2_hp = hp.LD(1) if ff is None else ac.s2_of(f, m - n)
            s2 = 1.0 if ff is None else np.sum(f ** 2) / (m - n)
            pieces = []
            for b in range(B):
                sl = slice(b * nb, (b + 1) * nb)
                pieces += ac.cov_pieces("block %d" % b, cov.block(b), cov.stderr[sl], s2 * R0[sl, sl], loc[b] * s2_hp, nb)
            sl = slice(B * nb, n)
            pieces += ac.cov_pieces("shared", cov.shared, cov.stderr[sl], s2 * R0[sl, sl], shared * s2_hp, ng)
            ac.judge("covariance bordered %s nb=%d ng=%d B=%d%s%s" % (family, nb, ng, B, label, flabel), pieces)


# ------------------------------------------------------------------------------------------ 6. dense Cholesky(), damped
def dense_pieces(op, x, damp):
    A = hp.ld(op.J)
    n = A.shape[1]
    x_hp = hp.normal_solve(A, op.y, damp)
    G = op.J.T @ op.J
    if damp is not None:
        G = G + np.diag(damp)
    S = ac.colnorms(A)
    return [("x", ac.solve_err(x, x_hp, S), ac.solve_err(np.linalg.solve(G, op.J.T @ op.y), x_hp, S), n)]


@pytest.mark.parametrize("family", ["plain", "graded", "ill"])
@pytest.mark.parametrize("n", [9, 70, 129, 200])
def test_dense_cholesky_damped(ctx, n, family):
    """The one-workgroup, blocked and one-launch paths (test_b_gpu_kernels.py::test_ldiv_cholesky names them the same way)."""
    op = ac.dense_operand(family, 3 * n + 5, n, 30 + n)
    x, sv = solve(ctx, lsq.DeviceMatrix(ctx, op.J), op.y, op.damp)
    assert sv.info()["chol_path"] == ("blocked-one-launch" if n >= 128 else "blocked" if n >= 32 else "one-workgroup")
    ac.judge("dense damped %s n=%d" % (family, n), dense_pieces(op, x, op.damp))


# ------------------------------------------------------------------------------------------ 7. dense Dogleg Cholesky()
@pytest.mark.parametrize("family", ["plain", "graded"])
def test_dense_cholesky_dogleg(ctx, family):
    op = ac.dense_operand(family, 400, 96, 96)
    x, sv = solve(ctx, lsq.DeviceMatrix(ctx, op.J), op.y, None)
    path = sv.info()["chol_path"]
    assert path in ("blocked-certified", "one-workgroup")
    ac.judge("dense dogleg %s (%s)" % (family, path), dense_pieces(op, x, None))


# ------------------------------------------------------------------------------------------ 8. dense QR panel
@pytest.mark.parametrize("c", [1, 5, 7, 7.75])
def test_dense_qr_panel(ctx, c, monkeypatch):
    """640 x 64, singular values logspace(0, -c, 64): ||Q1'Q1 - I||_F of the first CholeskyQR pass is about 1e-15, 4e-7, 1e-3, 6e-2
    (an fp64 stand-in on the CPU), which selects the first-order, series, second-Cholesky and near-gate branches of cq_factor<2>."""
    m, n = 640, 64
    rng = np.random.default_rng(int(100 * c))
    A = ac.ill_matrix(rng, m, n, decades=c)
    y = rng.standard_normal(m)
    monkeypatch.setenv("LSQ_QR_TWO_STAGE", "1")
    x, sv = solve(ctx, lsq.DeviceMatrix(ctx, A), y, None, solver=lsq.QR(), for_lm=False)
    info = sv.info()
    assert info["qr_rank"] == n
    if c <= 5:
        assert info["qr_panel"] == "cholqr2"
    x_hp = hp.lstsq_qr(A, y)
    S = ac.colnorms(A)
    e_ref = min(ac.solve_err(np.linalg.lstsq(A, y, rcond=None)[0], x_hp, S), ac.solve_err(ac.qr_fp64_solve(A, y), x_hp, S))
    ac.judge("dense qr c=%s (%s)" % (c, info["qr_panel"]), [("x", ac.solve_err(x, x_hp, S), e_ref, n)])


# ------------------------------------------------------------------------------------------ 9. BlockQR(), graded
@pytest.mark.parametrize("damped", [False, True])
@pytest.mark.parametrize("mb,nb", [(40, 17), (257, 64)])
def test_blockqr_graded(ctx, mb, nb, damped):
    """Column j times 10^(-6 j/(nb-1)): far from rcond = nb eps, so every rank is nb -- the oracle's."""
    B = 4
    V = lsq.synthetic.blockdiag_inputs(B, mb, nb, 500 + mb + nb)
    J = lsq.BlockDiagonal(B, mb, nb, data=V * np.repeat(np.tile(ac.grading(nb, 6.0), B), mb))
    y = np.random.default_rng(mb + nb).standard_normal(B * mb)
    damp = 0.1 * ac.colsumabs2(J) if damped else None
    x, _, sv, _, _ = bq_solve(ctx, lsq.DeviceMatrix(ctx, J), y, damp)
    _, ranks = oracle_blocks(J, y, damp)
    assert np.all(ranks == nb) and np.array_equal(sv.info()["block_ranks"], ranks)
    pieces = []
    for b in range(B):
        A, yb = hp.ld(J.block(b)), hp.ld(y[b * mb:(b + 1) * mb])
        A64, y64 = J.block(b), y[b * mb:(b + 1) * mb]
        if damped:
            db = damp[b * nb:(b + 1) * nb]
            A, yb = np.vstack([A, np.diag(np.sqrt(hp.ld(db)))]), np.concatenate([yb, np.zeros(nb, dtype=hp.LD)])
            A64, y64 = np.vstack([A64, np.diag(np.sqrt(db))]), np.concatenate([y64, np.zeros(nb)])
        x_hp = hp.lstsq_qr(A, yb)
        S = ac.colnorms(J.block(b))
        # (the better of LAPACK's two: gelsd is not invariant under column scaling and loses two to three digits on graded columns)
        e_ref = min(ac.solve_err(np.linalg.lstsq(A64, y64, rcond=None)[0], x_hp, S), ac.solve_err(ac.qr_fp64_solve(A64, y64), x_hp, S))
        pieces.append(("block %d" % b, ac.solve_err(x[b * nb:(b + 1) * nb], x_hp, S), e_ref, nb))
    ac.judge("blockqr graded %dx%d %s" % (mb, nb, "damped" if damped else "undamped"), pieces)
