"""Rank-deficient accuracy tier, host part (no device): the operands, references and the rule of tests/rankdef_common.py are
certified here before tests/test_s_gpu_accuracy_rankdef.py relies on them.

1. The longdouble minimum-norm solves (tests/hp_reference.py) against each other, against the Moore-Penrose conditions and
   against numpy's pinv.
2. Family E, every committed case: both factors have full rank r and cond <= 1e3, the oracle alone finds rank r, and the
   rule accepts LAPACK's own dgelsy (blocked dgeqp3) and, where the columns share one scale, numpy's SVD minimum-norm
   solution (numpy.linalg.lstsq), while it rejects (a) the solution truncated at rank r - 1 and (b) the basic solution
   (zeros in the non-pivot columns, no minimum-norm completion) -- both computed in longdouble, so that nothing but the
   defect separates them from x_hp.  On columns spread over 4 / 8 decades the SVD is NOT accepted and is not asked to be:
   it is backward stable normwise, not column by column, and lands 20 to 1000 x further from x_hp than xGELSY does
   (30 x 12 over 8 decades: 9.1e-14 against 4.5e-15; 9 x 6: 3.0e-10 against 2.6e-13).
3. Family T, every committed case: the oracle alone returns the intended rank, LAPACK's dgelsy returns it too and passes the
   rule, and the rule rejects the rank decided with 100 rcond wherever that changes the rank (every deficient K = 30 case;
   of the just-full-rank ones 700 x 100 keeps rank 100 there -- dlaic1's estimate of sigma_min sits above 100 rcond -- and is
   then simply the right answer).  Measured |rho_orc - rho_hp|, from which the device's bound 16 max(., 64 * 2^-53) follows
   (rho_hp itself: 1.4e-12 .. 1.4e-9):
       40 x 33     r 20: 7.6e-16 / 1.4e-16 (K 30 / 1000)    r 33:  4.4e-17 / 5.5e-18        bound 1.14e-13 (the floor)
       700 x 100   r 37: 3.3e-16 / 8.7e-17                  r 100: 7.6e-16 / 1.8e-16        bound 1.14e-13
       900 x 100   r 37: 1.7e-14 / 2.1e-16                  r 100: 5.5e-16 / 4.5e-16        bound 2.75e-13 at r 37, K 30; else 1.14e-13
       2100 x 2049 r 5, K 30: 1.6e-14                                                       bound 2.55e-13
   A rank decided with 100 rcond moves rho by 2.4e-13 .. 2.7e-7.  The truncation at r - 1 and the basic solution are not asked
   of family T: rho is dominated by the component of x along sigma_r, and at 900 x 100, r 37, K 1000 the right-hand side happens
   to have next to none of it (|rho - rho_hp| = 3.1e-16 after truncation).
4. Family Z and the BlockQR batches: the oracle's ranks are the intended ones, its x is exactly 0.0 on the zero columns, and
   the rule accepts a second fp64 solution (numpy's Householder QR on the stacked operand without its zero columns).
5. The exact-Gram forms that serve operands with more than 400 columns agree with the Householder forms at 1000 x 321.
6. The shapes sit on the device paths they are meant for (the dispatch rule of lsq_qr_solve, restated)."""
import numpy as np
import pytest

import accuracy_common as ac
import hp_reference as hp
import rankdef_common as rc

LD = hp.LD


def nrm(v):
    v = hp.ld(v).reshape(-1)
    return float(np.sqrt(v @ v))


# ------------------------------------------------------------------------------------------ 1. the longdouble solves
@pytest.mark.parametrize("r,n", [(1, 7), (4, 10), (7, 12), (20, 33), (33, 33)])
def test_minnorm_solve_is_the_pseudo_inverse(r, n):
    rng = np.random.default_rng(r * n)
    W = rng.standard_normal((r, n))
    c = rng.standard_normal(r)
    z = hp.minnorm_solve(W, c)
    assert z.dtype == LD
    Wl = hp.ld(W)
    assert nrm(Wl @ z - c) <= 8 * n * 2.0 ** -63 * (nrm(Wl) * nrm(z) + nrm(c))          # it solves W z = c
    # ... and lies in the row space: z = W'u for some u, i.e. z is orthogonal to the null space (projector from numpy's SVD)
    _, _, Vt = np.linalg.svd(W)
    assert nrm(Vt[r:] @ z.astype(np.float64)) <= 1e-13 * nrm(z)
    assert rc.rel_err(hp.minnorm_gram_solve(W, c), z) <= 1e-15
    assert rc.rel_err(np.linalg.pinv(W) @ c, z) <= 1e-12


def test_minnorm_solve_on_graded_rows_where_the_gram_form_loses_digits():
    """W = C D over 8 decades, 5 x 6: cond(W W') is beyond 1e12, the Cholesky form carries that factor, the QR form does not --
    judged by the equations themselves, row-equilibrated."""
    op = rc.EOperand(9, 6, 5, "dec8")
    z = hp.lstsq_qr(op.B, op.y0)
    x_qr, x_ch = hp.minnorm_solve(op.W, z), hp.minnorm_gram_solve(op.W, z)
    assert nrm(op.W @ x_qr - z) <= 8 * 6 * 2.0 ** -63 * (nrm(op.W) * nrm(x_qr) + nrm(z))
    print("QR form against Gram form at 8 decades: %.3e" % rc.rel_err(x_ch, x_qr))
    assert rc.rel_err(x_ch, x_qr) <= 1e-6            # the same solution, as far as the Gram form can tell


def test_pivoted_truncated_solve_full_rank_is_lstsq_qr():
    rng = np.random.default_rng(5)
    A, y = rng.standard_normal((30, 9)), rng.standard_normal(30)
    jp = rng.permutation(9)
    assert rc.rel_err(hp.pivoted_truncated_solve(A, y, jp, 9), hp.lstsq_qr(A, y)) <= 1e-17
    assert np.all(hp.pivoted_truncated_solve(A, y, jp, 0) == 0)


# ------------------------------------------------------------------------------------------ 2. family E
def wrong_answers(A, y, jpvt, r):
    """(truncated at r - 1, basic solution), both in longdouble with the oracle's pivots."""
    basic = np.zeros(A.shape[1], dtype=LD)
    basic[jpvt[:r]] = hp.lstsq_qr(A[:, jpvt[:r]], y)
    return hp.pivoted_truncated_solve(A, y, jpvt, r - 1), basic


def second_solutions_accepted(A, y, r, decades, x_hp, e_ref, k, label):
    """LAPACK's own dgelsy (blocked dgeqp3: another realisation of the reference's algorithm) on every operand; numpy's SVD
    minimum-norm solution (lstsq: gelsd) where the columns share one scale -- an SVD is backward stable normwise, not
    column by column, and on columns spread over 4 / 8 decades it is 20 to 1000 x further from x_hp than xGELSY is (measured
    here: 9.1e-14 against 4.5e-15 at 30 x 12 over 8 decades), which is the SVD's property and not the rule's."""
    x, rank = rc.lapack_gelsy(A, y)
    assert rank == r, (label, rank)
    pieces = [("dgelsy", rc.rel_err(x, x_hp), e_ref, k)]
    if decades == 0:
        x, _, rank, _ = np.linalg.lstsq(A, y, rcond=None)
        assert rank == r, (label, rank)
        pieces.append(("numpy SVD", rc.rel_err(x, x_hp), e_ref, k))
    ac.judge(label, pieces)


def certify_e(ref, label):
    op = ref.op
    m, n, r = op.m, op.n, op.r
    cb, cc = op.factor_conds()
    assert np.linalg.matrix_rank(op.B.astype(float)) == r and np.linalg.matrix_rank(op.C.astype(float)) == r, label
    assert cb <= rc.COND_MAX and cc <= rc.COND_MAX, (label, cb, cc)
    assert ref.rank_orc == r, (label, ref.rank_orc)
    second_solutions_accepted(op.A, op.y, r, rc.DECADES[op.variant], ref.x_hp, ref.e_ref, n, "host E " + label)
    if r > rc.GRAM_FROM:                   # (700 Householder steps in longdouble, twice: the smaller cases make the point)
        return
    trunc, basic = wrong_answers(op.A, op.y, ref.jpvt, r)
    e_trunc, e_basic = rc.rel_err(trunc, ref.x_hp), rc.rel_err(basic, ref.x_hp)
    print("   e_ref %.3e bound %.3e | truncated at r - 1: %.3e | basic: %.3e" % (ref.e_ref, ac.bound(ref.e_ref, n), e_trunc, e_basic))
    assert not ac.accepted(e_trunc, ref.e_ref, n), (label, e_trunc)
    if n - len(op.zero_cols) > r:          # (otherwise no column is left out of the basis: the basic solution IS the minimum-norm one)
        assert not ac.accepted(e_basic, ref.e_ref, n), (label, e_basic)


E_ALL = rc.E_CASES + [rc.E_SWEEP_CASE] + [("default", m, n, r, v) for (m, n, r, v, _) in rc.E_DEFAULT_CASES]


@pytest.mark.parametrize("path,m,n,r,variant", E_ALL)
def test_family_e_case_is_certified(path, m, n, r, variant):
    certify_e(rc.e_ref(m, n, r, variant), "%s %dx%d r=%d %s" % (path, m, n, r, variant))


def test_far_variants_have_the_bits_of_plain():
    plain = rc.EOperand(30, 12, 7, "plain")
    for v, f in rc.FAR.items():
        far = rc.EOperand(30, 12, 7, v)
        assert np.array_equal(far.A, plain.A * f) and np.array_equal(far.y, plain.y * f)
        assert np.array_equal(rc.e_x_hp(far), rc.e_x_hp(plain))
        assert np.array_equal(hp.minnorm_from_factors(far.B, far.W, far.y0), rc.e_x_hp(plain))


def test_duplicate_and_zero_columns_are_what_they_say():
    op = rc.EOperand(30, 12, 7, "dup4")
    assert np.array_equal(op.A[:, 11], op.A[:, 0]) and np.any(op.A[:, 0] != 0)
    op = rc.EOperand(700, 100, 37, "zero2")
    assert not np.any(op.A[:, [1, 98]]) and np.count_nonzero(np.any(op.A != 0, axis=0)) == 98
    for dec, v in ((4, "dec4"), (8, "dec8")):
        d = rc.EOperand(30, 12, 7, v).d
        assert d.max() == 1.0 and 10.0 ** -dec / 2 < d.min() < 10.0 ** -dec * 2 and np.all(np.log2(d) == np.rint(np.log2(d)))


# ------------------------------------------------------------------------------------------ 3. family T
T_ALL = rc.T_CASES + [rc.T_SWEEP_CASE]


@pytest.mark.parametrize("path,m,n,r,K", T_ALL)
def test_family_t_case_is_certified(path, m, n, r, K):
    ref = rc.t_ref(m, n, r, K)
    label = "%s %dx%d r=%d K=%d" % (path, m, n, r, K)
    print("T %s | rank_orc %d rho_hp %.6e |rho_orc - rho_hp| %.3e bound %.3e"
          % (label, ref.rank_orc, float(ref.rho_hp), abs(float(ref.rho_orc - ref.rho_hp)), ref.bound))
    assert ref.rank_orc == r, (label, ref.rank_orc)
    assert ref.accepts(ref.x_orc)
    x2, rk2 = rc.lapack_gelsy(ref.A, ref.y)
    assert rk2 == r and ref.accepts(x2), (label, rk2, ref.dist(x2))
    if K == 30:
        x100, rk100, _ = rc.oracle_solve(ref.A, ref.y, rcond=100 * min(m, n) * rc.EPS)
        print("   rank with 100 rcond: %d, |rho - rho_hp| %.3e" % (rk100, ref.dist(x100)))
        # (just full rank: dlaic1's estimate of sigma_min from the pivoted triangle may sit above 100 rcond still; a deficient
        #  operand has sigma_r = 30 rcond on the diagonal's scale and must lose columns)
        assert rk100 < r or r == n, (label, rk100)
        if rk100 < r:
            assert not ref.accepts(x100), (label, rk100)


# ------------------------------------------------------------------------------------------ 4. family Z, BlockQR batches
def second_fp64_solution(zr):
    x = np.zeros(zr.n)
    if len(zr.keep):
        As, ys = ac.stacked(np.asarray(zr.A)[:, zr.keep], zr.y, zr.damp[zr.keep])
        x[zr.keep] = ac.qr_fp64_solve(As, ys)
    return x


@pytest.mark.parametrize("path,m,n,z,variant", rc.Z_CASES)
def test_family_z_case_is_certified(path, m, n, z, variant):
    zr = rc.z_ref(m, n, z, variant)
    zero = np.setdiff1d(np.arange(n), zr.keep)
    assert len(zero) == z and zr.rank_orc == n - z
    assert np.all(zr.x_orc[zero] == 0.0) and np.all(zr.x_orc[zr.keep] != 0.0)
    ac.judge("host Z %s %dx%d z=%d %s: numpy QR" % (path, m, n, z, variant), [("x", zr.err(second_fp64_solution(zr)), zr.e_ref, n)])
    print("   e_ref %.3e" % zr.e_ref)


@pytest.mark.parametrize("nb", rc.BQ_NBS)
@pytest.mark.parametrize("mb", rc.BQ_MBS)
def test_blockqr_batch_is_certified(mb, nb):
    blocks, damped = rc.bq_batch(mb, nb), rc.bq_damped_refs(mb, nb)
    assert [b.kind for b in blocks].count("zero") == 1 and [b.kind for b in blocks].count("T") == 1 and len(blocks) == 9
    for b, (blk, zr) in enumerate(zip(blocks, damped)):
        label = "blockqr %dx%d block %d (%s)" % (mb, nb, b, blk.kind)
        x, rk, jp = rc.oracle_solve(blk.A, blk.y)
        assert rk == blk.rank, (label, rk, blk.rank)
        nonzero = int(np.count_nonzero(np.any(blk.A != 0, axis=0)))
        assert zr.rank_orc == nonzero, (label, zr.rank_orc)
        if blk.kind == "zero":
            assert np.all(x == 0.0) and np.all(zr.x_orc == 0.0)
            continue
        if blk.kind == "T":
            assert blk.tref.accepts(x)
        else:
            e_ref = rc.rel_err(x, blk.x_hp)
            second_solutions_accepted(blk.A, blk.y, blk.rank, blk.decades, blk.x_hp, e_ref, nb, "host " + label)
            if blk.rank > 0:
                trunc, _ = wrong_answers(blk.A, blk.y, jp, blk.rank)
                assert not ac.accepted(rc.rel_err(trunc, blk.x_hp), e_ref, nb), label
        assert ac.accepted(zr.err(second_fp64_solution(zr)), zr.e_ref, nb), (label, "damped")


# ------------------------------------------------------------------------------------------ 5. the exact-Gram forms
def test_exact_gram_forms_agree_with_the_householder_forms():
    """rc._e_z / rc.e_x_hp / rc.z_ref switch to hp.normal_solve_refined and hp.minnorm_gram_refined beyond 400 columns.  At
    1000 x 321 (r = 300, cond(B) = 3.4, cond(C) = 61) and on the damped 700 x 200 operand both forms are affordable: they agree
    to 1e-17, three orders below anything fp64 can show."""
    op = rc.EOperand(1000, 321, 300, "plain")
    z = hp.lstsq_qr(op.B, op.y0)
    zg = hp.normal_solve_refined(op.B, op.y0, (op.B.T @ op.B).astype(LD))
    x, xg = hp.minnorm_solve(op.W, z), hp.minnorm_gram_refined(op.W, z, (op.C @ op.C.T).astype(LD))
    print("exact-Gram against Householder: z %.3e x %.3e" % (rc.rel_err(zg, z), rc.rel_err(xg, x)))
    assert rc.rel_err(zg, z) <= 1e-17 and rc.rel_err(xg, x) <= 1e-17
    zop = rc.EOperand(700, 200, 200, "dec4", seed=rc.e_seed(700, 200, 200) + 1, certify=False, zero_cols=rc.z_cols(200, 3))
    gram = (zop.P.T @ zop.P).astype(LD) * np.outer(hp.ld(zop.d), hp.ld(zop.d))
    a, b = rc.ZRef(zop.A, zop.y), rc.ZRef(zop.A, zop.y, gram)
    print("   damped: %.3e" % a.err(b.x_hp))
    assert a.err(b.x_hp) <= 1e-17


# ------------------------------------------------------------------------------------------ 6. the shapes and their paths
def test_shapes_sit_on_their_paths():
    for m, n, r in rc.ONE_WG:
        assert not rc.two_stage_by_default(m, n) and not rc.multi_cu(m, n)
    for m, n, r in rc.ONE_STAGE:
        assert rc.multi_cu(m, n)
    assert [m < n for m, n, _ in rc.ONE_STAGE] == [False, False, False, True]
    for p, m, n in rc.Z_SHAPES:                       # the stacked operand is (m + n) x n
        assert p == "two-stage" or rc.multi_cu(m + n, n) == (p == "one-stage"), (p, m, n)
        assert rc.z_env(p, m, n).get("LSQ_QR_ONE_STAGE") == "1" or not rc.two_stage_by_default(m + n, n) or p == "two-stage"
    assert rc.TWO_STAGE[2][1] >= 320 and rc.TWO_STAGE[3][1] >= 768 and rc.SWEEP[1] > 2048
    for m, n, r, v, path in rc.E_DEFAULT_CASES:
        assert rc.two_stage_by_default(m, n) == (path == "two-stage-pivoted")
