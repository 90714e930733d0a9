"""Accuracy tier on the device, dense part: the blocked QR beyond one panel (lsq_qr_stage1.hip, lsq_qr_cholqr.hip, lsq_qr.hip:
multi-panel CholeskyQR2, the Householder panel steps and their row-slab exchanges, TSQR, the pivoted and the one-stage paths,
every A/B switch of the trailing kernels) and the dense Cholesky past n = 200 (lsq_dense_mfma.hip: the one-launch chain over
four to six 64-column steps, the panel launches, the pair SYRK of tall thin operands), held to LAPACK's OWN error as
tests/test_h_gpu_accuracy.py holds the block solvers.  Runs after it.

The shape tier (test_b) guards these paths at rel 1e-9 .. 1e-8 on standard-normal operands with cond < 10 and a random
right-hand side.  Here, per case:
    x_hp     hp.lstsq_qr / hp.normal_solve (numpy.longdouble) on the effective operand; damped QR: the stacked
             [A; diag(sqrt(damp))] in longdouble
    metric   ac.solve_err with S = the column norms of A, one piece, k = n
    e_ref    QR cases: numpy.linalg.qr + a triangular solve in fp64 (ac.qr_fp64_solve); Cholesky cases: numpy.linalg.solve
             of the fp64 normal equations
    rule     ac.judge: e_dev <= 16 max(e_ref, 64 * 2^-53)
Operands: ac.dense_operand, families plain / graded (8 decades) / ill (cond 1e3) / far+ / far-, each with the family's
damping, and TWO right-hand sides: random, and consistent (y = fl(A (z / colnorms))).  The random one carries a large residual,
whose cond^2 u term enters every solver's error; the consistent one leaves a backward-stable QR at cond u and is the sharper
test of anything that squares the condition number (tests/test_accuracy_host.py: the rule rejects the fp64 normal equations
36 to 41 x beyond the bound there, 19 to 20 x on the random y).  Every case asserts the path it means to test from AllocatedSolver.info().  The seeds below were fixed before the first
device run; no case is skipped, expected to fail or reseeded.

One longdouble factorisation serves both right-hand sides and every path switch on the same operand (ac.qr_ref, chol_ref
below); far+ / far- reuse plain's x_hp: scaling operand and y by 2^100 (damping by 2^200) changes no bit of any quotient
(tests/test_accuracy_host.py::test_far_operand_has_the_bits_of_plain)."""
import functools

import numpy as np
import pytest

import accuracy_common as ac
import hp_reference as hp
from gpu_common import lsq

pytestmark = pytest.mark.gpu

RHS, qr_ref = ac.RHS, ac.qr_ref


def device_solve(ctx, A, y, damp, solver):
    Jd = lsq.DeviceMatrix(ctx, A)
    sv = lsq.AllocatedSolver(Jd, solver, for_lm=damp is not None)
    dx = lsq.DeviceVector(ctx, Jd.n)
    dd = lsq.DeviceVector(ctx, Jd.n, damp) if damp is not None else None
    sv.ldiv_(dx, lsq.DeviceVector(ctx, Jd.m, y), dd)
    x, info = dx.get(), sv.info()
    sv.free()
    Jd.free()
    return x, info


def run_qr(ctx, monkeypatch, family, m, n, rhs, damped, env, expect, label):
    """One QR() solve under the switches `env`; expect: the info() entries the case is about (qr_rank == n always)."""
    ref = qr_ref(family, m, n)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    x, info = device_solve(ctx, ref.A, ref.Y[:, RHS.index(rhs)], ref.damp if damped else None, lsq.QR())
    what = "%s %dx%d %s %s %s" % (label, m, n, family, rhs, "damped" if damped else "undamped")
    print("PATH %s | %s %s rank %s" % (what, info["qr_path"], info["qr_panel"], info["qr_rank"]))
    assert info["qr_rank"] == n, (what, info)
    for key, want in expect.items():
        assert info[key] == want, (what, key, info)
    ac.judge("qr " + what, [("x", ac.solve_err(x, ref.x_hp(rhs, damped), ref.S), ref.e_ref(rhs, damped), n)])


CERTIFIED_CHOLQR = {"qr_path": "two-stage-certified", "qr_panel": "cholqr2"}

# ------------------------------------------------------------------------------------------ a. multi-panel QR
# 640 x 128: two full panels; 700 x 130: two panels and a ragged two-column tail; 1000 x 321: five panels plus one column, odd
# leading dimension; 400 x 256: the fourth full-width panel has 400 - 192 = 208 rows, fewer than 256, so it takes the Householder
# steps inside a solve whose qr_panel still says cholqr2
PANEL_CASES = ac.cases(ac.QR_PANEL_SHAPES, ac.QR_PANEL_FAMILIES)


@pytest.mark.parametrize("m,n,family,rhs,damped", PANEL_CASES)
def test_qr_multi_panel(ctx, monkeypatch, m, n, family, rhs, damped):
    run_qr(ctx, monkeypatch, family, m, n, rhs, damped, {"LSQ_QR_TWO_STAGE": "1"}, CERTIFIED_CHOLQR, "panels")


# ------------------------------------------------------------------------------------------ b. every other path, one operand
TWO = {"LSQ_QR_TWO_STAGE": "1"}
PATH_SWITCHES = {
    "householder-panel": (dict(TWO, LSQ_QR1_NO_CHOLQR="1"), {"qr_path": "two-stage-certified", "qr_panel": "householder-steps"}),
    "always-pivot": (dict(TWO, LSQ_QR_ALWAYS_PIVOT="1"), {"qr_path": "two-stage-pivoted"}),
    "one-stage": ({"LSQ_QR_ONE_STAGE": "1"}, {"qr_path": "one-stage"}),
    "lds-update-and-vtb": (dict(TWO, LSQ_QR_UPDATE_W="0", LSQ_QR_VTB_W="0"), CERTIFIED_CHOLQR),
    "lookahead": (dict(TWO, LSQ_QR_LOOKAHEAD="1"), CERTIFIED_CHOLQR),
    "top-lu": (dict(TWO, LSQ_QR_TOP_LU="1"), CERTIFIED_CHOLQR),
    "no-fused-gram": (dict(TWO, LSQ_QR_NO_FUSED_GRAM="1"), CERTIFIED_CHOLQR),
}


@pytest.mark.parametrize("damped", [False, True])
@pytest.mark.parametrize("switch", list(PATH_SWITCHES))
@pytest.mark.parametrize("family", ["graded", "ill"])
def test_qr_every_other_path(ctx, monkeypatch, family, switch, damped):
    env, expect = PATH_SWITCHES[switch]
    run_qr(ctx, monkeypatch, family, 1000, 321, "consistent", damped, env, expect, switch)


# ------------------------------------------------------------------------------------------ c. row-count variants of the panel kernels
# n = 70 (one full panel and six columns).  Default path: the CholeskyQR passes over 47 .. 344 slabs of 64 rows; at 22000 rows
# the default look-ahead rule fires on a 256-CU device (m - 64 > 64 * 256).  Householder panel: one workgroup per column
# (LSQ_QR1_COOP=0: the looping kernel), 2 / 4 / 8 row slabs with the in-kernel exchange (<= 4096 / 8192 / 20480 rows), the
# looping kernel beyond
ROW_VARIANTS = {"default": ({}, CERTIFIED_CHOLQR),
                "householder coop": ({"LSQ_QR1_NO_CHOLQR": "1", "LSQ_QR1_COOP": "1"},
                                     {"qr_path": "two-stage-certified", "qr_panel": "householder-steps"}),
                "householder no coop": ({"LSQ_QR1_NO_CHOLQR": "1", "LSQ_QR1_COOP": "0"},
                                        {"qr_path": "two-stage-certified", "qr_panel": "householder-steps"})}


@pytest.mark.parametrize("variant", list(ROW_VARIANTS))
@pytest.mark.parametrize("family", ["graded", "ill"])
@pytest.mark.parametrize("m", ac.QR_ROW_VARIANT_MS)
def test_qr_panel_row_variants(ctx, monkeypatch, m, family, variant):
    env, expect = ROW_VARIANTS[variant]
    run_qr(ctx, monkeypatch, family, m, ac.QR_ROW_VARIANT_N, "consistent", False, env, expect, variant)


# ------------------------------------------------------------------------------------------ d. TSQR
# one shape per register template of the slab kernel (n <= 8, 12, 16, 20, 24, 28, 32), each just above the 32768-row threshold;
# 140000 x 31: the first level leaves ceil(140000 / 128) * 31 = 33914 stacked rows >= 32768, so a second level runs
TSQR_CASES = ac.cases(ac.QR_TSQR_SHAPES, ac.QR_TSQR_FAMILIES)
NO_TSQR_CASES = [c for c in TSQR_CASES if c[1] in (12, 31)]


@pytest.mark.parametrize("m,n,family,rhs,damped", TSQR_CASES)
def test_qr_tsqr(ctx, monkeypatch, m, n, family, rhs, damped):
    run_qr(ctx, monkeypatch, family, m, n, rhs, damped, {}, {"qr_path": "two-stage-certified"}, "tsqr")


@pytest.mark.parametrize("m,n,family,rhs,damped", NO_TSQR_CASES)
def test_qr_tall_thin_generalised_exchange(ctx, monkeypatch, m, n, family, rhs, damped):
    """LSQ_QR_NO_TSQR=1: 16 / 64 / 256 row slabs per column with the generalised exchange."""
    run_qr(ctx, monkeypatch, family, m, n, rhs, damped, {"LSQ_QR_NO_TSQR": "1"}, {"qr_path": "two-stage-certified"}, "no-tsqr")


# ------------------------------------------------------------------------------------------ e. dense Cholesky past n = 200
@functools.lru_cache(maxsize=4)
def chol_ref(family, m, n, damped):
    """(operand, x_hp, S, e_ref) of the (damped) normal equations, as test_h_gpu_accuracy.py::dense_pieces forms them."""
    op = ac.dense_operand(family, m, n, 30 + n)
    damp = op.damp if damped else None
    A = hp.ld(op.J)
    x_hp = hp.normal_solve(A, op.y, damp)
    G = op.J.T @ op.J
    if damped:
        G = G + np.diag(damp)
    S = ac.colnorms(A)
    return op, x_hp, S, ac.solve_err(np.linalg.solve(G, op.J.T @ op.y), x_hp, S)


def run_chol(ctx, monkeypatch, family, m, n, damped, env, path, label):
    op, x_hp, S, e_ref = chol_ref(family, m, n, damped)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    x, info = device_solve(ctx, op.J, op.y, op.damp if damped else None, lsq.Cholesky())
    what = "%s %dx%d %s" % (label, m, n, family)
    print("PATH %s | %s" % (what, info["chol_path"]))
    assert info["chol_path"] == path, (what, info)
    ac.judge("cholesky " + what, [("x", ac.solve_err(x, x_hp, S), e_ref, n)])


CHOL_SWITCHES = {"default": ({}, "blocked-one-launch"),                                # k_chol_chain: six steps at 321, ragged
                 "panel launches": ({"LSQ_CHOL_PANELS": "1"}, "blocked"),
                 "separate J'y": ({"LSQ_CHOL_SEPARATE_JTY": "1"}, "blocked-one-launch")}


@pytest.mark.parametrize("family", ["plain", "graded", "ill"])
@pytest.mark.parametrize("n", [256, 384])
def test_cholesky_one_launch_chain(ctx, monkeypatch, n, family):
    """k_chol_chain over four (256) and six (384) full 64-column steps with the fused forward solve, J'y riding in the SYRK launch;
    321 -- five full steps and a ragged one-column step -- is test_cholesky_321_and_its_switches."""
    run_chol(ctx, monkeypatch, family, 3 * n + 5, n, True, {}, "blocked-one-launch", "damped")


@pytest.mark.parametrize("switch", list(CHOL_SWITCHES))
@pytest.mark.parametrize("family", ["plain", "graded", "ill"])
def test_cholesky_321_and_its_switches(ctx, monkeypatch, family, switch):
    env, path = CHOL_SWITCHES[switch]
    run_chol(ctx, monkeypatch, family, 3 * 321 + 5, 321, True, env, path, "damped " + switch)


@pytest.mark.parametrize("family", ["plain", "graded", "ill"])
@pytest.mark.parametrize("m,n", [(20000, 12), (16384, 32)])
def test_cholesky_tall_thin_pair_syrk(ctx, monkeypatch, m, n, family):
    """k_syrk_small: the pair kernel of operands with few columns and many rows (blocked from m n >= 20000; below two 64-column
    blocks there is no one-launch chain)."""
    run_chol(ctx, monkeypatch, family, m, n, True, {}, "blocked", "damped tall")


@pytest.mark.parametrize("family,path", [("plain", "blocked-certified"), ("graded", "one-workgroup")])
def test_cholesky_dogleg_963x321(ctx, monkeypatch, family, path):
    """for_lm=False: the unpivoted blocked factorisation where its certificate 1 / ||inv(U)||_F^2 > 16 n eps max diag(J'J) holds.
    On graded it cannot: the last column is 1e-8 of the first, so lambda_min(J'J) <= 1e-16 max diag < 1.1e-12 max diag, and the
    pivoted one-workgroup kernel must run (as at 400 x 96 in test_h_gpu_accuracy.py::test_dense_cholesky_dogleg) -- asserted,
    so that neither case can silently test the other's path."""
    run_chol(ctx, monkeypatch, family, 963, 321, False, {}, path, "dogleg")
