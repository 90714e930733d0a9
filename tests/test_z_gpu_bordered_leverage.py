"""lsq_bordered_qr_leverage on the device (lsq_lev_bordered.hip: k_bl_local, k_bl_add around k_lev_tall and k_lev_diag, behind
the elimination of BorderedQR() and the factor of its inner QR()): the accuracy tier's rule with k = nb + ng on every kernel
edge and on the ill families; the sum of the leverages; agreement with lsq_dense_qr_leverage on the dense matrix; new rows;
bits; the derived outputs against the twin of k_lev_diag; the workspace it shares with solves and covariances; both LSQ_ERANK
kinds with reuse of the solver; every refusal; and the diagnostics of a global fit.

The rule, the reference (leverage_common.q_hp on the stacked dense matrix, longdouble), e_ref (leverage_common.q_fp64), the cases
and the numpy twin that certifies them without a device are in tests/bordered_leverage_common.py /
tests/test_bordered_leverage_host.py."""
import ctypes as C

import numpy as np
import pytest

import accuracy_common as ac
import bordered_leverage_common as blc
import borderedqr_common as bqc
import borderedqr_cov_common as bc
import hp_reference as hp
import leverage_common as lc
import schur_common as sc
from gpu_common import lsq

pytestmark = pytest.mark.gpu

EARG, ERANK = lsq._lib.EARG, lsq._lib.ERANK
KEYS = ("q", "se", "t", "cook", "s2")


def solver_on(ctx, J, colscale=None):
    Jd = lsq.DeviceMatrix(ctx, J)
    if colscale is not None:
        Jd.set_colscale(lsq.DeviceVector(ctx, Jd.n, colscale))
    return Jd, lsq.AllocatedSolver(Jd, lsq.BorderedQR(), for_lm=True)


def padded(ctx, A, ld):
    """A (p x k) on the device with leading dimension ld, NaN in the padding rows."""
    buf = np.full((ld, A.shape[1]), np.nan, order="F")
    buf[:A.shape[0]] = A
    return lsq.DeviceVector(ctx, buf.size, buf.reshape(-1, order="F"))


def raw(ctx, sv, Jd, f=None, block=0, Al=None, Ag=None, pad=0, want=KEYS):
    """lsq_bordered_qr_leverage through the C ABI.  Al, Ag: the p x nb and p x ng parts of new rows of `block`, uploaded with
    leading dimensions p + pad and p + 2 pad.  Returns (rc, dict of the outputs asked for, h_info[0], h_info[1])."""
    rows, p = Jd.m, 0
    dAl = dAg = None
    if Al is not None:
        p = rows = Al.shape[0]
        dAl, dAg = padded(ctx, Al, p + pad), padded(ctx, Ag, p + 2 * pad)
    df = lsq.DeviceVector(ctx, Jd.m, f) if f is not None else None
    out = {k: lsq.DeviceVector(ctx, rows, np.full(rows, -7.0)) for k in want if k != "s2"}
    s2 = C.c_double(-7.0)
    info = np.full(2, -5, dtype=np.int32)
    ptr = lambda k: out[k].ptr if k in out else None
    rc = lsq.lib().lsq_bordered_qr_leverage(sv.h, Jd.h, block, dAl.ptr if dAl else None, p + pad, dAg.ptr if dAg else None,
                                            p + 2 * pad, p, df.ptr if df else None, ptr("q"), ptr("se"), ptr("t"), ptr("cook"),
                                            C.byref(s2) if "s2" in want else None, info.ctypes.data_as(lsq._lib.c_ip))
    res = {k: v.get() for k, v in out.items()} if rc == 0 else {}
    if rc == 0 and "s2" in want:
        res["s2"] = s2.value
    return rc, res, int(info[0]), int(info[1])


def device_pieces(r, sv, name=""):
    """Without and (m > n) with the residual on J's own rows, as pieces for the rule."""
    a = sv.bordered_qr_leverage()
    assert a.q.shape == (r.m,) and a.se is None and a.rank == r.ng and a.nblocks == r.B and a.mb == r.mb
    out = blc.pieces(name + "unscaled", a.q, r)
    if r.m > r.n:
        b = sv.bordered_qr_leverage(f=r.f)
        assert np.array_equal(a.q, b.q) and b.rank == r.ng
        out += blc.pieces(name + "f", b.q, r, True, b.se)
    return out


def damped_solve(ctx, sv, Jd, y, damp):
    dx = lsq.DeviceVector(ctx, Jd.n)
    sv.ldiv_(dx, lsq.DeviceVector(ctx, Jd.m, y), lsq.DeviceVector(ctx, Jd.n, damp))
    return dx.get()


# ------------------------------------------------------------------------------------------ 1. accuracy, 2. the sum
@pytest.mark.parametrize("case", blc.CASES, ids=blc.case_id)
def test_accuracy_and_sum_of_leverages(ctx, case):
    """mb = 2, 3, 12, 33, 40, 70, 96, 100, 110, 130, 160 (ragged slabs), nb = 1, 5, 16, 17, 33, 64, ng = 1, 3, 31, 32, 48, 63,
    64, 65, 129, 200 (tile edges): the shapes of borderedqr_cov_common.CASES."""
    family, shape = case
    op, r = blc.operand(family, shape), blc.ref(family, shape)
    Jd, sv = solver_on(ctx, op.J)
    blc.judge("bordered qr leverage %s %s" % (family, shape), device_pieces(r, sv))
    assert sv.info()["blockdiag_path"] == "bordered-qr" and sv.info()["blockdiag_block"] == -1
    h = sv.bordered_qr_leverage().h
    e_ref = lc.lev_err(r.q_ref, r.q_hp)
    total, total_hp = float(np.sum(hp.ld(h))), float(np.sum(r.q_hp))
    print("SUM %s %s: sum h - n = %.3e, bound %.3e" % (family, shape, total - r.n, ac.bound(e_ref, r.k) * total_hp))
    assert abs(total - r.n) <= ac.bound(e_ref, r.k) * total_hp
    if family == "graded":
        Jd, sv = solver_on(ctx, op.V, op.s)
        blc.judge("bordered qr leverage %s %s colscale" % (family, shape), device_pieces(blc.ref(family, shape, True), sv))


# ------------------------------------------------------------------------------------------ 3. the dense entry
@pytest.mark.parametrize("case", [("plain", (3, 100, 17, 65)), ("plain", (4, 100, 33, 129)), ("ill6", (5, 96, 5, 3))], ids=blc.case_id)
def test_agrees_with_the_dense_entry(ctx, case):
    family, shape = case
    op, r = blc.operand(family, shape), blc.ref(family, shape)
    Jd, sv = solver_on(ctx, op.J)
    new = sv.bordered_qr_leverage(f=r.f)
    old = lsq.dense_qr_leverage(lsq.DeviceMatrix(ctx, np.asfortranarray(r.A)), f=r.f)
    e_ref = lc.lev_err(r.q_ref, r.q_hp)
    both = ac.bound(e_ref, r.k) + ac.bound(e_ref, r.n)
    d = float(np.max(np.abs(hp.ld(new.q) - hp.ld(old.q)) / r.q_hp))
    se_hp = np.sqrt(r.s2_hp * r.q_hp)
    e_ref_se = lc.lev_err(np.sqrt(r.s2 * r.q_ref), se_hp)
    dse = float(np.max(np.abs(hp.ld(new.se) - hp.ld(old.se)) / se_hp))
    print("AGREE dense %s %s: q %.3e of %.3e, se %.3e" % (family, shape, d, both, dse))
    assert d <= both and dse <= ac.bound(e_ref_se, r.k) + ac.bound(e_ref_se, r.n)
    assert new.s2 == old.s2


# ------------------------------------------------------------------------------------------ 4. new rows
@pytest.mark.parametrize("shape", [(3, 40, 5, 31), (3, 100, 17, 65)])
def test_new_rows(ctx, shape):
    """p = 1, 63, 64, 65, 130 (one lane of a slab, a slab less one, a full slab, one row into the second, into the third) on the
    first and the last block, tight and with padded leading dimensions (NaN in the padding)."""
    B, mb, nb, ng = shape
    op = blc.operand("plain", shape)
    J, f = op.J, op.y
    Jd, sv = solver_on(ctx, J)
    for b in (0, B - 1):
        for p in (1, 63, 64, 65, 130):
            Al, Ag = blc.new_rows(J, b, p, 100 * b + p)
            r = blc.Ref(op, A=blc.full_rows(J, b, Al, Ag))
            rc, tight, i0, i1 = raw(ctx, sv, Jd, f=f, block=b, Al=Al, Ag=Ag, want=("q", "se", "s2"))
            assert (rc, i0, i1) == (0, 0, ng)
            rc, pad, _, _ = raw(ctx, sv, Jd, f=f, block=b, Al=Al, Ag=Ag, pad=3, want=("q", "se", "s2"))
            assert rc == 0 and np.all(np.isfinite(tight["q"]))
            assert np.array_equal(tight["q"], pad["q"]) and np.array_equal(tight["se"], pad["se"]) and tight["s2"] == pad["s2"]
            blc.judge("bordered qr leverage new rows %s b=%d p=%d" % (shape, b, p), blc.pieces("rows", tight["q"], r, True, tight["se"]))
            assert np.array_equal(tight["se"], lc.diag_twin(tight["q"], np.zeros(p), tight["s2"], Jd.n)[0])
            py = sv.bordered_qr_leverage(f=f, block=b, A_local=Al, A_shared=Ag)
            assert np.array_equal(py.q, tight["q"]) and np.array_equal(py.se, tight["se"]) and py.studentized is None
            assert py.rank == ng and py.s2 == tight["s2"]
    # a block's own rows as new rows: the bits of the own-row call (the handle has no column scale)
    own = sv.bordered_qr_leverage()
    for b in range(B):
        rc, same, _, _ = raw(ctx, sv, Jd, block=b, Al=np.asfortranarray(J.block(b)), Ag=np.asfortranarray(J.border_block(b)), want=("q",))
        assert rc == 0 and np.array_equal(same["q"], own.block(b).q), b
    # a row's bits depend neither on p nor on where it stands among the rows
    b = B - 1
    Al, Ag = blc.new_rows(J, b, 130, 7)
    rc, full, _, _ = raw(ctx, sv, Jd, block=b, Al=Al, Ag=Ag, want=("q",))
    assert rc == 0
    for lo, hi_ in ((0, 1), (60, 70), (64, 130), (129, 130)):
        rc, part, _, _ = raw(ctx, sv, Jd, block=b, Al=np.asfortranarray(Al[lo:hi_]), Ag=np.asfortranarray(Ag[lo:hi_]), pad=2, want=("q",))
        assert rc == 0 and np.array_equal(part["q"], full["q"][lo:hi_]), (lo, hi_)
    perm = np.random.default_rng(3).permutation(130)
    rc, mixed, _, _ = raw(ctx, sv, Jd, block=b, Al=np.asfortranarray(Al[perm]), Ag=np.asfortranarray(Ag[perm]), want=("q",))
    assert rc == 0 and np.array_equal(mixed["q"], full["q"][perm])
    # ... nor on how the launch groups the border tiles: 148 copies of the rows are more slabs than the chip has CUs
    reps = 148
    rc, many, _, _ = raw(ctx, sv, Jd, block=b, Al=np.asfortranarray(np.tile(Al, (reps, 1))), Ag=np.asfortranarray(np.tile(Ag, (reps, 1))), want=("q",))
    assert rc == 0 and np.array_equal(many["q"], np.tile(full["q"], reps))


def test_more_new_rows_than_the_fit_has(ctx):
    """p > m on (1, 3, 1, 1): the scratch grows from call to call."""
    shape = (1, 3, 1, 1)
    op = blc.operand("plain", shape)
    Jd, sv = solver_on(ctx, op.J)
    first = None
    for p in (2, 200, 5):
        Al, Ag = blc.new_rows(op.J, 0, 200, 11)
        Al, Ag = np.asfortranarray(Al[:p]), np.asfortranarray(Ag[:p])
        got = sv.bordered_qr_leverage(f=op.y, block=0, A_local=Al, A_shared=Ag)
        r = blc.Ref(op, A=blc.full_rows(op.J, 0, Al, Ag))
        blc.judge("bordered qr leverage p=%d > m=3" % p, blc.pieces("rows", got.q, r, True, got.se))
        first = got.q if first is None else first
        assert np.array_equal(got.q[:2], first[:2])


# ------------------------------------------------------------------------------------------ 5. bits
@pytest.mark.parametrize("shape", [(65, 12, 5, 64), (3, 100, 17, 65), (5, 110, 64, 200)])
def test_bits(ctx, shape):
    op = blc.operand("plain", shape)
    Jd, sv = solver_on(ctx, op.J)
    f = op.y
    same = lambda x, y: all(np.array_equal(x[k], y[k]) for k in KEYS)
    rc, a, i0, i1 = raw(ctx, sv, Jd, f=f)
    assert (rc, i0, i1) == (0, 0, shape[3]) and all(np.all(np.isfinite(a[k])) for k in KEYS)
    rc, b, _, _ = raw(ctx, sv, Jd, f=f)
    assert rc == 0 and same(a, b)
    lsq.debug_set(serial=1)
    try:
        rc, ser, _, _ = raw(ctx, sv, Jd, f=f)
    finally:
        lsq.debug_set(serial=0)
    assert rc == 0 and same(a, ser)
    lsq.debug_set(launch_jitter_us=200)
    try:
        rc, jit, _, _ = raw(ctx, sv, Jd, f=f)
    finally:
        lsq.debug_set(launch_jitter_us=0)
    assert rc == 0 and same(a, jit)
    Jd2, sv2 = solver_on(ctx, op.J)
    rc, other, _, _ = raw(ctx, sv2, Jd2, f=f)
    assert rc == 0 and same(a, other)
    # every combination of outputs, d_q = NULL included (the solver's own buffer)
    for mask in range(1, 32):
        want = tuple(k for i, k in enumerate(KEYS) if mask >> i & 1)
        rc, sub, _, _ = raw(ctx, sv, Jd, f=f, want=want)
        assert rc == 0 and set(sub) == set(want) and all(np.array_equal(sub[k], a[k]) for k in want), want
    rc, qonly, _, _ = raw(ctx, sv, Jd, want=("q",))
    assert rc == 0 and np.array_equal(qonly["q"], a["q"])


# ------------------------------------------------------------------------------------------ 6. derived outputs
@pytest.mark.parametrize("shape", [(3, 85, 5, 31), (2, 128, 16, 64), (3, 100, 17, 65)])
def test_derived_outputs_bit_for_bit(ctx, shape):
    """se, t and cook from the device's own q and s2 and the numpy twin of k_lev_diag: equal bits; m = 255, 256 and 300 (one
    workgroup of k_lev_diag less one row, exactly one, into the second)."""
    B, mb, nb, ng = shape
    J = sc.make_bb(B, mb, nb, ng, 17)
    f = np.random.default_rng(mb).standard_normal(B * mb)
    Jd, sv = solver_on(ctx, J)
    rc, d, _, _ = raw(ctx, sv, Jd, f=f)
    assert rc == 0
    se, t, cook = lc.diag_twin(d["q"], f, d["s2"], Jd.n)
    assert np.array_equal(d["se"], se) and np.array_equal(d["t"], t) and np.array_equal(d["cook"], cook)
    assert all(np.all(np.isfinite(d[k])) for k in KEYS)
    py = sv.bordered_qr_leverage(f=f)
    assert py.s2 == d["s2"] and np.array_equal(py.cook, d["cook"]) and np.array_equal(py.studentized, d["t"])
    blk = py.block(B - 1)
    assert blk.s2 == py.s2 and blk.info is None and np.array_equal(blk.h, d["q"][(B - 1) * mb:]) and blk.cook.shape == (mb,)


# ------------------------------------------------------------------------------------------ 7. the shared workspace
def test_solves_and_covariances_around_a_leverage_keep_their_bits(ctx):
    shape = (3, 100, 17, 65)
    op = blc.operand("plain", shape)
    f = op.y
    Jd, sv = solver_on(ctx, op.J)
    Jd2, plain = solver_on(ctx, op.J)
    x0 = damped_solve(ctx, plain, Jd2, op.y, op.damp)
    cov0 = plain.bordered_qr_covariance(f=f, cross=True)
    lev1 = sv.bordered_qr_leverage(f=f)
    assert np.array_equal(damped_solve(ctx, sv, Jd, op.y, op.damp), x0)        # a solve after a leverage
    sv.bordered_qr_leverage(f=f)
    cov1 = sv.bordered_qr_covariance(f=f, cross=True)                          # a covariance after a leverage
    assert np.array_equal(cov1.cov, cov0.cov) and np.array_equal(cov1.stderr, cov0.stderr) and np.array_equal(cov1.cross, cov0.cross)
    lev0 = plain.bordered_qr_leverage(f=f)                                     # a leverage after a covariance: W and F are shared
    lev2 = sv.bordered_qr_leverage(f=f)
    for k in ("q", "se", "studentized", "cook"):
        assert np.array_equal(getattr(lev0, k), getattr(lev1, k)) and np.array_equal(getattr(lev2, k), getattr(lev1, k)), k
    assert lev0.s2 == lev1.s2 and np.array_equal(damped_solve(ctx, plain, Jd2, op.y, op.damp), x0)


# ------------------------------------------------------------------------------------------ 8. failures
def _clean_call_afterwards(ctx, sv, Jd):
    K, yk, dk, _ = bqc.rank_case("good")
    Jd.set_values(K.data)
    r = blc.Ref(ac.Operand(K, yk, dk))
    blc.judge("bordered qr leverage after a failure", device_pieces(r, sv))
    assert sv.info()["blockdiag_block"] == -1
    assert sc.rel_err(damped_solve(ctx, sv, Jd, yk, dk), bqc.qr_fp64_reference(K, yk, dk)) <= sc.SOLVE_RTOL
    cv = sv.bordered_qr_covariance(f=yk, cross=True)
    ac.judge("bordered qr covariance after a failing leverage", bc.Ref(ac.Operand(K, yk, dk)).pieces(bc.Parts.of_dev(cv), True))


@pytest.mark.parametrize("name", bqc.RANK_CASES)
def test_failing_local_column(ctx, name):
    J, y, _, expect = bqc.rank_case(name)
    assert expect > 0
    Jd, sv = solver_on(ctx, J)
    rc, _, i0, _ = raw(ctx, sv, Jd, f=y)
    msg = lsq.lib().lsq_last_error().decode()
    assert rc == ERANK and i0 == expect, (name, rc, i0, msg)
    assert msg == bqc.ERANK_TEXT % expect
    assert sv.info()["blockdiag_block"] == (expect - 1) // J.nb
    with pytest.raises(lsq.RankDeficientException) as e:
        sv.bordered_qr_leverage()
    assert e.value.status == ERANK and str(e.value) == bqc.ERANK_TEXT % expect
    _clean_call_afterwards(ctx, sv, Jd)


def test_rank_deficient_border(ctx):
    J = bc.duplicated_border_case()
    ng = J.ng
    Jd, sv = solver_on(ctx, J)
    rc, _, i0, i1 = raw(ctx, sv, Jd, want=("q",))
    msg = lsq.lib().lsq_last_error().decode()
    print("duplicated border column ->", rc, i0, i1, msg)
    assert rc == ERANK and i0 == 0 and i1 == ng - 1
    assert "RankDeficientException" in msg and "rank %d" % (ng - 1) in msg and "ng = %d" % ng in msg
    with pytest.raises(lsq.RankDeficientException):
        sv.bordered_qr_leverage()
    K = sc.make_bb(J.nblocks, J.mb, J.nb, ng, 5)
    Jd.set_values(K.data)
    rng = np.random.default_rng(9)
    f, damp = rng.standard_normal(Jd.m), 0.05 + rng.random(Jd.n)
    blc.judge("bordered qr leverage after a rank-deficient border", device_pieces(blc.Ref(ac.Operand(K, f, damp)), sv))
    assert sc.rel_err(damped_solve(ctx, sv, Jd, f, damp), bqc.qr_fp64_reference(K, f, damp)) <= sc.SOLVE_RTOL


def test_refusals(ctx):
    import scipy.sparse as sp
    L = lsq.lib()
    rng = np.random.default_rng(3)
    J = sc.make_bb(3, 8, 2, 4, 1)                          # 24 x 10
    bb, qr = solver_on(ctx, J)
    o = lsq.DeviceVector(ctx, 4096).ptr
    f = lsq.DeviceVector(ctx, 64, rng.standard_normal(64)).ptr
    rl, rs = lsq.DeviceVector(ctx, 64).ptr, lsq.DeviceVector(ctx, 64).ptr
    dense = lsq.DeviceMatrix(ctx, rng.standard_normal((24, 10)))
    csc = lsq.DeviceMatrix(ctx, sp.random(24, 10, 0.5, format="csc", random_state=1))
    bd = lsq.DeviceMatrix(ctx, lsq.BlockDiagonal(3, 8, 2, data=lsq.synthetic.blockdiag_inputs(3, 8, 2, 1)))
    wide, qr_wide = solver_on(ctx, sc.make_bb(2, 2, 3, 1, 1))           # 4 x 7
    square, qr_sq = solver_on(ctx, sc.make_bb(1, 2, 1, 1, 1))           # 2 x 2
    s2 = C.c_double(0.0)
    N = None
    # (label, solver, handle, block, d_Ab, ldab, d_Ag, ldag, p, d_f, d_q, d_se, d_student, d_cook, h_s2, fragment)
    cases = [
        ("every output NULL", qr, bb, 0, N, 0, N, 0, 0, f, N, N, N, N, N, "all NULL"),
        ("a Cholesky() solver", lsq.AllocatedSolver(bb, lsq.Cholesky(), for_lm=True), bb, 0, N, 0, N, 0, 0, N, o, N, N, N, N, "needs a BorderedQR() solver"),
        ("a Schur() solver", lsq.AllocatedSolver(bb, lsq.Schur(), for_lm=True), bb, 0, N, 0, N, 0, 0, N, o, N, N, N, N, "needs a BorderedQR() solver"),
        ("an LSMR() solver", lsq.AllocatedSolver(bb, lsq.LSMR(), for_lm=True), bb, 0, N, 0, N, 0, 0, N, o, N, N, N, N, "needs a BorderedQR() solver"),
        ("a dense QR() solver", lsq.AllocatedSolver(dense, lsq.QR(), for_lm=False), dense, 0, N, 0, N, 0, 0, N, o, N, N, N, N, "lsq_dense_qr_leverage"),
        ("a dense handle", qr, dense, 0, N, 0, N, 0, 0, N, o, N, N, N, N, "lsq_dense_qr_leverage"),
        ("a plain CSC handle", qr, csc, 0, N, 0, N, 0, 0, N, o, N, N, N, N, "lsq_sparse_covariance"),
        ("a block-diagonal handle", qr, bd, 0, N, 0, N, 0, 0, N, o, N, N, N, N, "lsq_solver_leverage"),
        ("more shared columns", qr, lsq.DeviceMatrix(ctx, sc.make_bb(3, 8, 2, 5, 1)), 0, N, 0, N, 0, 0, N, o, N, N, N, N, "create a solver on the handle"),
        ("more blocks", qr, lsq.DeviceMatrix(ctx, sc.make_bb(4, 8, 2, 4, 1)), 0, N, 0, N, 0, 0, N, o, N, N, N, N, "3 blocks of 8 x 2 with 4 shared columns"),
        ("m < n", qr_wide, wide, 0, N, 0, N, 0, 0, N, o, N, N, N, N, "needs m >= n"),
        ("m = n with f", qr_sq, square, 0, N, 0, N, 0, 0, f, o, N, N, N, N, "pass d_f = NULL"),
        ("se without f", qr, bb, 0, N, 0, N, 0, 0, N, o, o, N, N, N, "need the residual d_f"),
        ("student without f", qr, bb, 0, N, 0, N, 0, 0, N, N, N, o, N, N, "need the residual d_f"),
        ("cook without f", qr, bb, 0, N, 0, N, 0, 0, N, N, N, N, o, N, "need the residual d_f"),
        ("s2 without f", qr, bb, 0, N, 0, N, 0, 0, N, o, N, N, N, C.byref(s2), "need the residual d_f"),
        ("student with new rows", qr, bb, 0, rl, 2, rs, 2, 2, f, o, N, o, N, N, "must be NULL"),
        ("cook with new rows", qr, bb, 0, rl, 2, rs, 2, 2, f, o, N, N, o, N, "must be NULL"),
        ("only the local parts", qr, bb, 0, rl, 2, N, 2, 2, N, o, N, N, N, N, "need both parts"),
        ("only the shared parts", qr, bb, 0, N, 2, rs, 2, 2, N, o, N, N, N, N, "need both parts"),
        ("block < 0", qr, bb, -1, rl, 2, rs, 2, 2, N, o, N, N, N, N, "0 <= block < B = 3"),
        ("block = B", qr, bb, 3, rl, 2, rs, 2, 2, N, o, N, N, N, N, "0 <= block < B = 3"),
        ("p < 1", qr, bb, 0, rl, 4, rs, 4, 0, N, o, N, N, N, N, "p >= 1, ldab >= p and ldag >= p"),
        ("ldab < p", qr, bb, 0, rl, 3, rs, 4, 4, N, o, N, N, N, N, "p >= 1, ldab >= p and ldag >= p"),
        ("ldag < p", qr, bb, 0, rl, 4, rs, 3, 4, N, o, N, N, N, N, "p >= 1, ldab >= p and ldag >= p"),
    ]
    for label, sv, Jh, blk, pl, ldl, pg, ldg, p, pf, pq, pse, pt, pck, ps2, fragment in cases:
        rc = L.lsq_bordered_qr_leverage(sv.h, Jh.h, blk, pl, ldl, pg, ldg, p, pf, pq, pse, pt, pck, ps2, None)
        msg = L.lsq_last_error().decode()
        print(label, "->", rc, msg)
        assert rc == EARG, (label, rc)
        assert msg.startswith("lsq_bordered_qr_leverage:") and fragment in msg, (label, msg)
    with pytest.raises(lsq.ArgumentError) as ea:                           # ... and as the Python exception
        lsq.AllocatedSolver(bb, lsq.Schur(), for_lm=True).bordered_qr_leverage()
    assert ea.value.status == EARG and "needs a BorderedQR() solver" in str(ea.value)
    for refused in (dense, csc, bd):                                       # (no BorderedQR() solver exists on these handles)
        with pytest.raises(lsq.ArgumentError):
            lsq.bordered_qr_leverage(refused)
    with pytest.raises(lsq.ArgumentError):
        qr.bordered_qr_leverage(block=0, A_local=np.zeros((2, 2)))
    # the older entries name the new one where they refuse a bordered handle
    chol = lsq.AllocatedSolver(bb, lsq.Cholesky(), for_lm=True)
    assert L.lsq_solver_leverage(chol.h, bb.h, N, o, N, N, N, N, None) == EARG
    assert "lsq_bordered_qr_leverage" in L.lsq_last_error().decode()
    # the solvers work after the refusals; the function that owns its solver gives the same bits
    rf = rng.standard_normal(24)
    r = blc.Ref(ac.Operand(J, rf, None))
    blc.judge("bordered qr leverage after refusals", device_pieces(r, qr))
    one, again = lsq.bordered_qr_leverage(bb, f=rf), qr.bordered_qr_leverage(f=rf)
    for k in ("q", "se", "studentized", "cook"):
        assert np.array_equal(getattr(one, k), getattr(again, k)), k
    # m = n without f is served: every leverage is 1
    hsq = qr_sq.bordered_qr_leverage().h
    assert hsq.shape == (2,) and np.all(np.abs(hsq - 1.0) <= 1e-12)
    damp = 0.05 + rng.random(10)
    assert sc.rel_err(damped_solve(ctx, qr, bb, rf, damp), bqc.qr_fp64_reference(J, rf, damp)) <= sc.SOLVE_RTOL


def test_through_ctypes(ctx):
    shape = (3, 40, 5, 31)
    B, mb, nb, ng = shape
    op, r = blc.operand("plain", shape), blc.ref("plain", shape)
    L = lsq.lib()
    m = B * mb
    Jh, sh = C.c_void_p(), C.c_void_p()
    assert L.lsq_blockdiag_bordered_create(ctx.h, B, mb, nb, ng, C.byref(Jh)) == 0
    vals = np.ascontiguousarray(op.J.data, dtype=np.float64)
    assert L.lsq_mat_set_values(Jh, vals.ctypes.data_as(C.POINTER(C.c_double))) == 0
    assert L.lsq_solver_create(ctx.h, Jh, lsq._lib.BORDERED_QR, 1, C.byref(sh)) == 0
    df = lsq.DeviceVector(ctx, m, r.f)
    dq, dse, dt, dck = (lsq.DeviceVector(ctx, m) for _ in range(4))
    s2 = C.c_double(0.0)
    info = (C.c_int * 2)(-1, -1)
    assert L.lsq_bordered_qr_leverage(sh, Jh, 0, None, 0, None, 0, 0, df.ptr, dq.ptr, dse.ptr, dt.ptr, dck.ptr, C.byref(s2),
                                      info) == 0, L.lsq_last_error().decode()
    assert (info[0], info[1]) == (0, ng)
    blc.judge("bordered qr leverage through ctypes", blc.pieces("own", dq.get(), r, True, dse.get()))
    se, t, cook = lc.diag_twin(dq.get(), r.f, s2.value, B * nb + ng)
    assert np.array_equal(dt.get(), t) and np.array_equal(dck.get(), cook) and np.array_equal(dse.get(), se)
    # new rows of block 2 with raw pointers
    Al, Ag = blc.new_rows(op.J, 2, 9, 1)
    dl, dg = padded(ctx, Al, 9), padded(ctx, Ag, 12)
    dq9 = lsq.DeviceVector(ctx, 9)
    assert L.lsq_bordered_qr_leverage(sh, Jh, 2, dl.ptr, 9, dg.ptr, 12, 9, None, dq9.ptr, None, None, None, None, None) == 0
    blc.judge("bordered qr leverage new rows through ctypes", blc.pieces("rows", dq9.get(), blc.Ref(op, A=blc.full_rows(op.J, 2, Al, Ag))))
    assert L.lsq_solver_destroy(sh) == 0 and L.lsq_mat_destroy(Jh) == 0


# ------------------------------------------------------------------------------------------ 9. after a global fit
def test_diagnostics_after_a_global_fit(ctx):
    """B exponential decays a_b exp(-k t) + c_b that share the rate k, LevenbergMarquardt(BorderedQR()); then leverages,
    studentized residuals and Cook's distances at the solution and the standard error of curve 1 at abscissae that were not
    measured, against the longdouble reference on the Jacobian there."""
    B, mb, nb, ng = 6, 30, 2, 1
    t = np.linspace(0.0, 4.0, mb)
    rng = np.random.default_rng(42)
    a, c0, k = 1.0 + rng.random(B), 0.2 * rng.random(B), 0.8
    data = a[:, None] * np.exp(-k * t) + c0[:, None] + 0.01 * rng.standard_normal((B, mb))

    def model(x, tt):
        return x[0:2 * B:2, None] * np.exp(-x[2 * B] * tt) + x[1:2 * B:2, None]

    def f_(out, x):
        out[:] = (model(x, t) - data).reshape(-1)

    def rows(x, b, tt):
        e = np.exp(-x[2 * B] * tt)
        return np.asfortranarray(np.column_stack([e, np.ones_like(tt)])), np.asfortranarray((-x[2 * b] * tt * e)[:, None])

    def g_(J, x):
        for b in range(B):
            J.block(b)[:, :], J.border_block(b)[:, :] = rows(x, b, t)

    nls = lsq.LeastSquaresProblem(x=np.concatenate([np.tile([1.0, 0.0], B), [1.0]]), y=np.zeros(B * mb), f_=f_, g_=g_,
                                  J=lsq.BorderedBlockDiagonal(B, mb, nb, ng))
    res = lsq.optimize_(nls, lsq.LevenbergMarquardt(lsq.BorderedQR()), iterations=200, ctx=ctx)
    assert res.converged
    x = np.array(res.minimizer)
    assert abs(x[2 * B] - k) < 0.05
    Jf, fcur = lsq.BorderedBlockDiagonal(B, mb, nb, ng), np.zeros(B * mb)
    g_(Jf, x)
    f_(fcur, x)
    op = ac.Operand(Jf, fcur, None)
    r = blc.Ref(op)
    Jd = lsq.DeviceMatrix(ctx, Jf)
    lev = lsq.bordered_qr_leverage(Jd, f=fcur)
    blc.judge("bordered qr leverage after a global fit", blc.pieces("own", lev.q, r, True, lev.se))
    # t and cook: the twin's bits from the device's q and s2, and the longdouble values on the reference's q and s2.  With
    # bnd the rule's bound on e(q) and amp = max h / (1 - h) on the reference: d = 1 - h has e(d) <= amp bnd;
    # t = f / (sd sqrt(d)) has e(t) <= e(d) / 2 + e(s2) / 2 + five roundings <= (amp + 1) / 2 bnd (the variance, a sum of
    # m = 180 squares, and the roundings are far below the floor of bnd, 256 u); cook = t^2 h / (n d) has
    # e(cook) <= 2 e(t) + e(q) + e(d) <= (2 amp + 2) bnd
    se, tt, cook = lc.diag_twin(lev.q, fcur, lev.s2, r.n)
    assert np.array_equal(lev.studentized, tt) and np.array_equal(lev.cook, cook)
    assert np.all(lev.h > 0) and np.all(lev.h < 1)
    _, t_hp, cook_hp = lc.diag_hp(r.q_hp, fcur, r.s2_hp, r.n)
    bnd = ac.bound(lc.lev_err(r.q_ref, r.q_hp), r.k)
    amp = float(np.max(r.q_hp / (1 - r.q_hp)))
    e_t = float(np.max(np.abs(hp.ld(lev.studentized) - t_hp) / np.abs(t_hp)))
    e_c = float(np.max(np.abs(hp.ld(lev.cook) - cook_hp) / cook_hp))
    print("t: e %.3e of %.3e | cook: e %.3e of %.3e | amp %.2f" % (e_t, (amp + 1) / 2 * bnd, e_c, (2 * amp + 2) * bnd, amp))
    assert e_t <= (amp + 1) / 2 * bnd and e_c <= (2 * amp + 2) * bnd
    assert abs(lev.h.sum() - r.n) <= 1e-12 and np.all(np.abs(lev.studentized) < 5) and np.all(lev.cook >= 0)
    # the band of curve 1 beyond and between the measured abscissae
    Al, Ag = rows(x, 1, np.linspace(-0.5, 6.0, 23))
    band = lsq.bordered_qr_leverage(Jd, f=fcur, block=1, A_local=Al, A_shared=Ag)
    blc.judge("bordered qr leverage band of curve 1", blc.pieces("band", band.q, blc.Ref(op, A=blc.full_rows(Jf, 1, Al, Ag)), True, band.se))
    print("fit k %.4f | se of curve 1 %.3e .. %.3e | max leverage %.3f max |t| %.2f max cook %.3f"
          % (x[2 * B], band.se.min(), band.se.max(), lev.h.max(), np.abs(lev.studentized).max(), lev.cook.max()))
    assert np.all(band.se < 0.1)
