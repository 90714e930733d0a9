"""lsq_bordered_qr_covariance on the device (lsq_cov_bordered.hip: k_bqc_tsolve, k_bqc_tall, k_bqc_block, k_bqc_shared behind
the elimination of BorderedQR() and lsq_dense_qr_covariance on its inner QR()): the accuracy tier's rule on every kernel
branch and on the ill families, where a covariance that forms J'J is outside it; agreement with lsq_solver_covariance and
lsq_sparse_covariance on well-conditioned operands (the latter for the cross-covariances); bits; both LSQ_ERANK kinds with
reuse of the solver; every refusal; the standard errors of a fit; and one call with raw pointers.

The rule, the reference (longdouble Householder of the stacked dense matrix), e_ref (LAPACK's fp64 Householder route), the
cases and the numpy twin that certifies them without a device are in tests/borderedqr_cov_common.py /
tests/test_borderedqr_covariance_host.py."""
import ctypes as C

import numpy as np
import pytest

import accuracy_common as ac
import borderedqr_common as bqc
import borderedqr_cov_common as bc
import schur_common as sc
from gpu_common import lsq

pytestmark = pytest.mark.gpu

EARG, ERANK = lsq._lib.EARG, lsq._lib.ERANK


def solver_on(ctx, J, colscale=None):
    Jd = lsq.DeviceMatrix(ctx, J)
    if colscale is not None:
        Jd.set_colscale(lsq.DeviceVector(ctx, Jd.n, colscale))
    return Jd, lsq.AllocatedSolver(Jd, lsq.BorderedQR(), for_lm=True)


def raw_call(ctx, sv, Jd, f, want_cov, want_se, want_cross):
    """lsq_bordered_qr_covariance through the C ABI: (rc, cov, stderr, cross, h_info[0], h_info[1]); an output that was not
    asked for, or any after a failure, is None."""
    B, _, nb, ng = Jd.bordered
    dcov = lsq.DeviceVector(ctx, B * nb * nb + ng * ng) if want_cov else None
    dse = lsq.DeviceVector(ctx, Jd.n) if want_se else None
    dcr = lsq.DeviceVector(ctx, B * nb * ng) if want_cross else None
    df = lsq.DeviceVector(ctx, Jd.m, f) if f is not None else None
    info = np.full(2, -5, dtype=np.int32)
    rc = lsq.lib().lsq_bordered_qr_covariance(sv.h, Jd.h, df.ptr if df else None, dcov.ptr if dcov else None,
                                              dse.ptr if dse else None, dcr.ptr if dcr else None,
                                              info.ctypes.data_as(lsq._lib.c_ip))
    get = lambda d: d.get() if d is not None and rc == 0 else None
    return rc, get(dcov), get(dse), get(dcr), int(info[0]), int(info[1])


def device_pieces(ref, sv, with_f):
    cv = sv.bordered_qr_covariance(f=ref.f if with_f else None, cross=True)
    assert cv.rank == ref.ng and cv.info is None
    return ref.pieces(bc.Parts.of_dev(cv), with_f)


def damped_solve(ctx, sv, Jd, y, damp):
    dx = lsq.DeviceVector(ctx, Jd.n)
    sv.ldiv_(dx, lsq.DeviceVector(ctx, Jd.m, y), lsq.DeviceVector(ctx, Jd.n, damp))
    return dx.get()


# ------------------------------------------------------------------------------------------ 1. the rule on every branch and family
@pytest.mark.parametrize("case", bc.CASES, ids=bc.case_id)
def test_accuracy(ctx, case):
    family, shape = case
    op, ref = bc.operand(family, shape), bc.ref(family, shape)
    Jd, sv = solver_on(ctx, op.J)
    for with_f in (False, True):
        pieces = device_pieces(ref, sv, with_f)
        assert len(pieces) == 3 * shape[0] + 2
        ac.judge("bordered qr covariance %s %s%s" % (family, shape, " with f" if with_f else ""), pieces)
    assert sv.info()["blockdiag_path"] == "bordered-qr" and sv.info()["blockdiag_block"] == -1
    if family == "graded":
        Jd, sv = solver_on(ctx, op.V, op.s)
        ac.judge("bordered qr covariance %s %s colscale" % (family, shape), device_pieces(bc.ref(family, shape, True), sv, False))


# ------------------------------------------------------------------------------------------ 2. where it matters
def test_six_decades_where_the_cholesky_covariance_is_outside_the_rule(ctx):
    """ill6 (5, 96, 5, 3), nb + ng <= 64, cond(J'J) = 1e12: lsq_solver_covariance with Cholesky() on the same handle misses the
    bound or reports PosDefException; the new entry is inside."""
    shape = (5, 96, 5, 3)
    op, ref = bc.operand("ill6", shape), bc.ref("ill6", shape)
    Jd, sv = solver_on(ctx, op.J)
    ac.judge("bordered qr covariance ill6 %s" % (shape,), device_pieces(ref, sv, False))
    try:
        old = lsq.AllocatedSolver(Jd, lsq.Cholesky(), for_lm=True).covariance()
        over = bc.beyond(ref.pieces(bc.Parts.of_dev(old), False))
    except lsq.PosDefException:
        over = np.inf
    print("   lsq_solver_covariance (Cholesky()) on the same handle: %.3g x the bound" % over)
    assert over > 1.0


# ------------------------------------------------------------------------------------------ 3. agreement with the older entries
def _agree(ref, new, old, R_old, label):
    """new / old: Parts (unit variance); within the sum of both sides' bounds, piece by piece: the new entry's e_ref is the fp64
    Householder route, the old one's the inverse of the fp64 Gram matrix its own tests hold it to."""
    pn = {n: (r, k) for n, _, r, k in ref.pieces(new, False)}
    po = {n: (r, k) for n, _, r, k in ref.pieces(old, False, e_ref_of=R_old)}
    ac.judge(label + " (new entry)", ref.pieces(new, False))
    dist = ref.distances(new, old, False)
    assert dist
    for name, d in dist:
        both = ac.bound(*pn[name]) + ac.bound(*po[name])
        assert d <= both, (label, name, d, both)
    worst = max(dist, key=lambda t: t[1] / (ac.bound(*pn[t[0]]) + ac.bound(*po[t[0]])))
    print("AGREE %s | %d pieces | worst %s: %.3e of %.3e" % (label, len(dist), worst[0], worst[1],
                                                          ac.bound(*pn[worst[0]]) + ac.bound(*po[worst[0]])))
    return [n for n, _ in dist]


def test_agrees_with_the_cholesky_covariance(ctx):
    shape = (5, 96, 5, 3)
    op = bc.operand("plain", shape)
    ref = bc.ref("plain", shape)
    Jd, sv = solver_on(ctx, op.J)
    new = bc.Parts.of_dev(sv.bordered_qr_covariance())
    old = bc.Parts.of_dev(lsq.AllocatedSolver(Jd, lsq.Cholesky(), for_lm=True).covariance())
    names = _agree(ref, new, old, np.linalg.inv(ref.A.T @ ref.A), "vs lsq_solver_covariance plain %s" % (shape,))
    assert "block 0" in names and "shared" in names and "shared stderr" in names


def test_agrees_with_the_sparse_covariance_cross_blocks_included(ctx):
    shape = (3, 40, 5, 31)
    op, ref = bc.operand("plain", shape), bc.ref("plain", shape)
    Jd, sv = solver_on(ctx, op.J)
    new = bc.Parts.of_dev(sv.bordered_qr_covariance(cross=True))
    full = lsq.AllocatedSolver(Jd, lsq.LSMR(), for_lm=True).sparse_covariance()
    old = bc.Parts.of_full(full.cov, ref.B, ref.nb, ref.ng)
    old.stderr = full.stderr
    names = _agree(ref, new, old, np.linalg.inv(ref.A.T @ ref.A), "vs lsq_sparse_covariance plain %s" % (shape,))
    assert "cross 0" in names and "cross 2" in names


# ------------------------------------------------------------------------------------------ 4. bits
@pytest.mark.parametrize("shape", [(65, 12, 5, 64), (3, 100, 17, 65)])
def test_bits(ctx, shape):
    B, mb, nb, ng = shape
    op, ref = bc.operand("plain", shape), bc.ref("plain", shape)
    Jd, sv = solver_on(ctx, op.J)
    a = sv.bordered_qr_covariance(f=ref.f, cross=True)
    assert all(np.all(np.isfinite(v)) for v in (a.cov, a.stderr, a.cross))
    same = lambda c: np.array_equal(a.cov, c.cov) and np.array_equal(a.stderr, c.stderr) and np.array_equal(a.cross, c.cross)
    assert same(sv.bordered_qr_covariance(f=ref.f, cross=True))                       # the same solver again
    assert same(solver_on(ctx, op.J)[1].bordered_qr_covariance(f=ref.f, cross=True))   # a second solver, a second handle
    lsq.debug_set(serial=1)
    try:
        ser = sv.bordered_qr_covariance(f=ref.f, cross=True)
    finally:
        lsq.debug_set(serial=0)
    lsq.debug_set(launch_jitter_us=200)
    try:
        jit = sv.bordered_qr_covariance(f=ref.f, cross=True)
    finally:
        lsq.debug_set(launch_jitter_us=0)
    assert same(ser) and same(jit)
    # every diagonal block is symmetric to the bit
    for b in range(B):
        assert np.array_equal(a.block(b), a.block(b).T)
    assert np.array_equal(a.shared, a.shared.T)
    # stderr: the same bits for every combination of outputs; cov and cross do not depend on their company either
    for want_cov in (True, False):
        for want_cross in (True, False):
            rc, cov, se, cross, i0, i1 = raw_call(ctx, sv, Jd, ref.f, want_cov, True, want_cross)
            assert (rc, i0, i1) == (0, 0, ng)
            assert np.array_equal(se, a.stderr), (want_cov, want_cross)
            assert cov is None or np.array_equal(cov, a.cov)
            assert cross is None or np.array_equal(cross.reshape((B * nb, ng), order="F"), a.cross)
    rc, cov, _, cross, _, _ = raw_call(ctx, sv, Jd, ref.f, True, False, True)
    assert rc == 0 and np.array_equal(cov, a.cov) and np.array_equal(cross.reshape((B * nb, ng), order="F"), a.cross)
    rc, _, _, cross, _, _ = raw_call(ctx, sv, Jd, ref.f, False, False, True)
    assert rc == 0 and np.array_equal(cross.reshape((B * nb, ng), order="F"), a.cross)
    # sqrt(diag(cov)) to rounding: two sums of at most nb + ng terms in different orders, s^2 and the root
    diag = np.concatenate([np.diag(a.block(b)) for b in range(B)] + [np.diag(a.shared)])
    assert np.all(np.abs(a.stderr - np.sqrt(diag)) <= (2 * (nb + ng) + 8) * ac.UNIT * a.stderr)


def test_a_solve_after_a_covariance_has_the_bits_of_a_solve_without_one(ctx):
    shape = (3, 100, 17, 65)
    op = bc.operand("plain", shape)
    Jd, sv = solver_on(ctx, op.J)
    Jd2, sv2 = solver_on(ctx, op.J)
    x1 = damped_solve(ctx, sv, Jd, op.y, op.damp)
    sv.bordered_qr_covariance(f=op.y, cross=True)
    x2 = damped_solve(ctx, sv, Jd, op.y, op.damp)
    y1 = damped_solve(ctx, sv2, Jd2, op.y, op.damp)
    y2 = damped_solve(ctx, sv2, Jd2, op.y, op.damp)
    assert np.array_equal(x1, y1) and np.array_equal(x2, y2)
    assert sc.rel_err(x2, bqc.qr_fp64_reference(op.J, op.y, op.damp)) <= sc.SOLVE_RTOL
    assert sv.info()["qr_rank"] == Jd.n


# ------------------------------------------------------------------------------------------ 5. LSQ_ERANK and reuse
def _clean_call_afterwards(ctx, sv, Jd):
    K, yk, dk, _ = bqc.rank_case("good")
    Jd.set_values(K.data)
    ref = bc.Ref(ac.Operand(K, yk, dk))
    ac.judge("bordered qr covariance after a failure", device_pieces(ref, sv, True))
    assert sv.info()["blockdiag_block"] == -1
    assert sc.rel_err(damped_solve(ctx, sv, Jd, yk, dk), bqc.qr_fp64_reference(K, yk, dk)) <= sc.SOLVE_RTOL


@pytest.mark.parametrize("name", bqc.RANK_CASES)
def test_failing_local_column(ctx, name):
    J, y, _, expect = bqc.rank_case(name)
    assert expect > 0
    Jd, sv = solver_on(ctx, J)
    rc, _, _, _, i0, _ = raw_call(ctx, sv, Jd, y, True, True, True)
    msg = lsq.lib().lsq_last_error().decode()
    assert rc == ERANK and i0 == expect, (name, rc, i0, msg)
    assert msg == bqc.ERANK_TEXT % expect
    assert sv.info()["blockdiag_block"] == (expect - 1) // J.nb
    with pytest.raises(lsq.RankDeficientException) as e:
        sv.bordered_qr_covariance()
    assert e.value.status == ERANK and str(e.value) == bqc.ERANK_TEXT % expect
    _clean_call_afterwards(ctx, sv, Jd)


def test_rank_deficient_border(ctx):
    J = bc.duplicated_border_case()
    ng = J.ng
    Jd, sv = solver_on(ctx, J)
    rc, _, _, _, i0, i1 = raw_call(ctx, sv, Jd, None, True, True, True)
    msg = lsq.lib().lsq_last_error().decode()
    print("duplicated border column ->", rc, i0, i1, msg)
    assert rc == ERANK and i0 == 0 and i1 == ng - 1
    assert "RankDeficientException" in msg and "rank %d" % (ng - 1) in msg and "ng = %d" % ng in msg
    with pytest.raises(lsq.RankDeficientException):
        sv.bordered_qr_covariance(cov=False)
    # the same solver on an operand of full rank, then a solve
    K = sc.make_bb(J.nblocks, J.mb, J.nb, ng, 5)
    Jd.set_values(K.data)
    rng = np.random.default_rng(9)
    f, damp = rng.standard_normal(Jd.m), 0.05 + rng.random(Jd.n)
    ac.judge("bordered qr covariance after a rank-deficient border", device_pieces(bc.Ref(ac.Operand(K, f, damp)), sv, True))
    assert sc.rel_err(damped_solve(ctx, sv, Jd, f, damp), bqc.qr_fp64_reference(K, f, damp)) <= sc.SOLVE_RTOL


# ------------------------------------------------------------------------------------------ 6. refusals through the C ABI
def test_refusals(ctx):
    import scipy.sparse as sp
    L = lsq.lib()
    rng = np.random.default_rng(3)
    J = sc.make_bb(3, 8, 2, 4, 1)                          # 24 x 10, nb + ng <= 64
    bb, qr = solver_on(ctx, J)
    out = lsq.DeviceVector(ctx, 4096)
    f = lsq.DeviceVector(ctx, 64)
    dense = lsq.DeviceMatrix(ctx, rng.standard_normal((24, 10)))
    csc = lsq.DeviceMatrix(ctx, sp.random(24, 10, 0.5, format="csc", random_state=1))
    bd = lsq.DeviceMatrix(ctx, lsq.BlockDiagonal(3, 8, 2, data=lsq.synthetic.blockdiag_inputs(3, 8, 2, 1)))
    wide, qr_wide = solver_on(ctx, sc.make_bb(2, 2, 3, 1, 1))           # 4 x 7
    square, qr_sq = solver_on(ctx, sc.make_bb(1, 2, 1, 1, 1))           # 2 x 2
    cases = [
        ("all outputs NULL", qr, bb, None, None, None, None, "all NULL"),
        ("a Cholesky() solver", lsq.AllocatedSolver(bb, lsq.Cholesky(), for_lm=True), bb, None, out.ptr, None, None, "lsq_solver_covariance"),
        ("a Schur() solver", lsq.AllocatedSolver(bb, lsq.Schur(), for_lm=True), bb, None, out.ptr, None, None, "needs a BorderedQR() solver"),
        ("an LSMR() solver", lsq.AllocatedSolver(bb, lsq.LSMR(), for_lm=True), bb, None, None, out.ptr, None, "lsq_sparse_covariance"),
        ("a dense QR() solver", lsq.AllocatedSolver(dense, lsq.QR(), for_lm=False), dense, None, out.ptr, None, None, "lsq_dense_qr_covariance"),
        ("a dense handle", qr, dense, None, out.ptr, None, None, "lsq_dense_qr_covariance"),
        ("a plain CSC handle", qr, csc, None, None, None, out.ptr, "lsq_sparse_covariance"),
        ("a block-diagonal handle", qr, bd, None, out.ptr, None, None, "lsq_solver_covariance"),
        ("more shared columns", qr, lsq.DeviceMatrix(ctx, sc.make_bb(3, 8, 2, 5, 1)), None, out.ptr, None, None, "create a solver on the handle"),
        ("more blocks", qr, lsq.DeviceMatrix(ctx, sc.make_bb(4, 8, 2, 4, 1)), None, out.ptr, None, None, "3 blocks of 8 x 2 with 4 shared columns"),
        ("m < n", qr_wide, wide, None, out.ptr, out.ptr, None, "needs m >= n"),
        ("m < n with f", qr_wide, wide, f.ptr, None, None, out.ptr, "needs m >= n"),
        ("m = n with f", qr_sq, square, f.ptr, out.ptr, out.ptr, out.ptr, "pass d_f = NULL"),
    ]
    for label, sv, Jh, pf, pcov, pse, pcr, fragment in cases:
        rc = L.lsq_bordered_qr_covariance(sv.h, Jh.h, pf, pcov, pse, pcr, None)
        msg = L.lsq_last_error().decode()
        print(label, "->", rc, msg)
        assert rc == EARG, (label, rc)
        assert msg.startswith("lsq_bordered_qr_covariance:") and fragment in msg, (label, msg)
    with pytest.raises(lsq.ArgumentError) as ea:                           # ... and as the Python exception
        lsq.AllocatedSolver(bb, lsq.Schur(), for_lm=True).bordered_qr_covariance()
    assert ea.value.status == EARG and "needs a BorderedQR() solver" in str(ea.value)
    for refused in (dense, csc, bd):                                       # (no BorderedQR() solver exists on these handles)
        with pytest.raises(lsq.ArgumentError):
            lsq.bordered_qr_covariance(refused)
    # the solvers work after the refusals; m = n without f is served
    rf = rng.standard_normal(24)
    ref = bc.Ref(ac.Operand(J, rf, None))
    ac.judge("bordered qr covariance after refusals", device_pieces(ref, qr, True))
    one = lsq.bordered_qr_covariance(bb, f=rf, cross=True)                 # the function that owns its solver
    again = qr.bordered_qr_covariance(f=rf, cross=True)
    assert np.array_equal(one.cov, again.cov) and np.array_equal(one.stderr, again.stderr) and np.array_equal(one.cross, again.cross)
    sq = qr_sq.bordered_qr_covariance(cross=True)
    assert all(np.all(np.isfinite(v)) for v in (sq.cov, sq.stderr, sq.cross))
    damp = 0.05 + rng.random(10)
    assert sc.rel_err(damped_solve(ctx, qr, bb, rf, damp), bqc.qr_fp64_reference(J, rf, damp)) <= sc.SOLVE_RTOL


# ------------------------------------------------------------------------------------------ 7. after a fit
def test_standard_errors_and_cross_blocks_after_a_fit(ctx):
    """LevenbergMarquardt(BorderedQR()) on the graded tanh fit, then the covariance at the solution with the residual there,
    against the longdouble reference on the Jacobian at that point."""
    B, mb, nb, ng = sc.FITS[0]
    fit = bqc.GradedTanhFit(B, mb, nb, ng)
    r = lsq.optimize_(fit.bordered_problem(), lsq.LevenbergMarquardt(lsq.BorderedQR()), iterations=200, ctx=ctx)
    assert r.converged
    x = np.array(r.minimizer)
    J, fcur = lsq.BorderedBlockDiagonal(B, mb, nb, ng), np.zeros(fit.m)
    fit.fill(J, x)
    fit.f_(fcur, x)
    cv = lsq.bordered_qr_covariance(lsq.DeviceMatrix(ctx, J), f=fcur, cross=True)
    assert cv.rank == ng and cv.cross.shape == (B * nb, ng) and cv.cross_block(1).shape == (nb, ng)
    assert np.array_equal(cv.cross_block(1), cv.cross[nb:2 * nb])
    ac.judge("bordered qr covariance after a fit", bc.Ref(ac.Operand(J, fcur, None)).pieces(bc.Parts.of_dev(cv), True))
    assert np.all(np.isfinite(cv.stderr)) and np.all(cv.stderr > 0.0)


# ------------------------------------------------------------------------------------------ 8. raw pointers
def test_through_ctypes(ctx):
    shape = (3, 40, 5, 31)
    B, mb, nb, ng = shape
    op, ref = bc.operand("plain", shape), bc.ref("plain", shape)
    L = lsq.lib()
    m, n = B * mb, B * nb + ng
    Jh, sh = C.c_void_p(), C.c_void_p()
    assert L.lsq_blockdiag_bordered_create(ctx.h, B, mb, nb, ng, C.byref(Jh)) == 0
    vals = np.ascontiguousarray(op.J.data, dtype=np.float64)
    assert L.lsq_mat_set_values(Jh, vals.ctypes.data_as(C.POINTER(C.c_double))) == 0
    assert L.lsq_solver_create(ctx.h, Jh, lsq._lib.BORDERED_QR, 1, C.byref(sh)) == 0
    df = lsq.DeviceVector(ctx, m, ref.f)
    dcov, dse, dcr = lsq.DeviceVector(ctx, B * nb * nb + ng * ng), lsq.DeviceVector(ctx, n), lsq.DeviceVector(ctx, B * nb * ng)
    info = (C.c_int * 2)(-1, -1)
    assert L.lsq_bordered_qr_covariance(sh, Jh, df.ptr, dcov.ptr, dse.ptr, dcr.ptr, info) == 0, L.lsq_last_error().decode()
    assert (info[0], info[1]) == (0, ng)
    cov = dcov.get()
    parts = bc.Parts([cov[b * nb * nb:(b + 1) * nb * nb].reshape(nb, nb) for b in range(B)], cov[B * nb * nb:].reshape(ng, ng),
                     dse.get(), dcr.get().reshape((B * nb, ng), order="F"))
    ac.judge("bordered qr covariance through ctypes", ref.pieces(parts, True))
    assert L.lsq_solver_destroy(sh) == 0 and L.lsq_mat_destroy(Jh) == 0
