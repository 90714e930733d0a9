"""Parameter covariance of a dense Jacobian from the QR() factor on the device (lsq_dense_qr_covariance, lsq_cov_dense.hip: the
factorisation lsq_ldiv enqueues, X = inv(R) -- the certificate's, or lsq_tri_inv_enqueue on the pivoted triangle -- then
k_cov_xxt / k_cov_stderr or their un-permuting variants).  Operands, the longdouble reference (a Householder R, not J'J) and
the fp64 e_ref are in tests/qr_cov_common.py; the rule is the accuracy tier's, unchanged:
    ac.judge(ac.cov_pieces(.., k = n)): e_dev <= 16 max(e_ref, min(max(16, n), 64) 2^-53), covariance and stderr
tests/test_dense_qr_covariance_host.py shows on the CPU that two fp64 QR routes stay inside it on every case here and that the
normal equations do not on the ill-conditioned ones."""
import numpy as np
import pytest

import accuracy_common as ac
import hp_reference as hp
import qr_cov_common as qc
from gpu_common import lsq

pytestmark = pytest.mark.gpu

EARG, ERANK = lsq._lib.EARG, lsq._lib.ERANK


def solver_on(ctx, A, for_lm=False):
    Jd = lsq.DeviceMatrix(ctx, A)
    return Jd, lsq.AllocatedSolver(Jd, lsq.QR(), for_lm=for_lm)


def device_pieces(r, sv, name=""):
    """Both calls (without and with the residual) on one solver, as pieces for ac.judge."""
    pieces = []
    for with_f in (False, True):
        cov = sv.dense_qr_covariance(f=r.f if with_f else None)
        assert cov.n == r.n and cov.cov.shape == (r.n, r.n) and cov.stderr.shape == (r.n,)
        pieces += r.pieces(name + ("f" if with_f else "unscaled"), cov.cov, cov.stderr, with_f)
    return pieces


# ------------------------------------------------------------------------------------------ 1. accuracy
@pytest.mark.parametrize("m,n,family", qc.CASES)
def test_accuracy(ctx, m, n, family):
    r = qc.ref(family, m, n)
    Jd, sv = solver_on(ctx, r.A)
    before = sv.stats()["cholqr_panel"]["giveups"]
    pieces = device_pieces(r, sv)
    info = sv.info()
    print("PATH dense qr covariance %dx%d %s | %s %s rank %s | cholqr give-ups %d"
          % (m, n, family, info["qr_path"], info["qr_panel"], info["qr_rank"], sv.stats()["cholqr_panel"]["giveups"] - before))
    assert info["qr_rank"] == n
    ac.judge("dense qr covariance %s %dx%d" % (family, m, n), pieces)
    sv.free()
    Jd.free()


# ------------------------------------------------------------------------------------------ 2. every path
TWO = {"LSQ_QR_TWO_STAGE": "1"}
PATH_SWITCHES = {
    "two-stage": (TWO, {"qr_path": "two-stage-certified", "qr_panel": "cholqr2"}),
    "householder-panel": (dict(TWO, LSQ_QR1_NO_CHOLQR="1"), {"qr_path": "two-stage-certified", "qr_panel": "householder-steps"}),
    "always-pivot": (dict(TWO, LSQ_QR_ALWAYS_PIVOT="1"), {"qr_path": "two-stage-pivoted"}),
    "one-stage": ({"LSQ_QR_ONE_STAGE": "1"}, {"qr_path": "one-stage"}),
}
PIVOTED = ("always-pivot", "one-stage")


def check_permutation_was_applied(r, m, n, cov):
    """shuffled-graded on a pivoted path: the first pivot is the column of largest norm, the graded operand's column 0, which
    the shuffle has moved to position p0 != 0.  An un-permuted X X' would put H[p0, p0] where H[0, 0] belongs; the graded
    diagonal of H spans 16 decades, so the two differ by far more than the factor asked for here."""
    p0 = int(np.argmax(ac.colnorms(r.A).astype(float)))
    assert p0 != 0 and int(np.argsort(qc.shuffle_perm(m, n))[0]) == p0
    h00, hpp = float(r.H[0, 0]), float(r.H[p0, p0])
    assert max(h00, hpp) > 4 * min(h00, hpp)
    assert abs(cov.cov[0, 0] - h00) <= 0.01 * h00
    assert abs(cov.cov[0, 0] - hpp) > 0.5 * hpp
    assert abs(cov.stderr[0] ** 2 - hpp) > 0.5 * hpp


def run_path(ctx, monkeypatch, m, n, family, env, expect, label, for_lm=False):
    r = qc.ref(family, m, n)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    Jd, sv = solver_on(ctx, r.A, for_lm=for_lm)
    pieces = device_pieces(r, sv)
    cov = sv.dense_qr_covariance()
    info = sv.info()
    what = "%s %dx%d %s for_lm=%d" % (label, m, n, family, for_lm)
    print("PATH dense qr covariance %s | %s %s rank %s" % (what, info["qr_path"], info["qr_panel"], info["qr_rank"]))
    for key, want in expect.items():
        assert info[key] == want, (what, key, info)
    ac.judge("dense qr covariance " + what, pieces)
    sv.free()
    Jd.free()
    return r, cov


@pytest.mark.parametrize("switch", list(PATH_SWITCHES))
@pytest.mark.parametrize("family", ["plain", "shuffled-graded"])
@pytest.mark.parametrize("m,n", [(300, 65), (500, 130)])
def test_every_path(ctx, monkeypatch, m, n, family, switch):
    env, expect = PATH_SWITCHES[switch]
    r, cov = run_path(ctx, monkeypatch, m, n, family, env, expect, switch)
    if family == "shuffled-graded" and switch in PIVOTED:
        check_permutation_was_applied(r, m, n, cov)


@pytest.mark.parametrize("family", ["plain", "shuffled-graded"])
def test_no_tsqr(ctx, monkeypatch, family):
    run_path(ctx, monkeypatch, 33000, 8, family, {"LSQ_QR_NO_TSQR": "1"}, {"qr_path": "two-stage-certified"}, "no-tsqr")


@pytest.mark.parametrize("family", ["plain", "shuffled-graded"])
def test_one_stage_multi_cu(ctx, monkeypatch, family):
    """The one-stage switch sends 300 x 65 and 500 x 130 to the one-workgroup kernel (M n < 65536); the stacked 900 x 200 of a
    for_lm solver is the smallest of the shapes that reaches the multi-CU pivoted Householder, R at leading dimension M = m + n."""
    m, n = 700, 200
    r, cov = run_path(ctx, monkeypatch, m, n, family, {"LSQ_QR_ONE_STAGE": "1"}, {"qr_path": "one-stage"}, "one-stage multi-CU",
                      for_lm=True)
    if family == "shuffled-graded":
        check_permutation_was_applied(r, m, n, cov)


# ------------------------------------------------------------------------------------------ 3. bits
def raw_call(ctx, sv, Jd, f, want_cov, want_se):
    """lsq_dense_qr_covariance through the C ABI: (rc, cov or None, stderr or None, h_info)."""
    n = Jd.n
    dcov = lsq.DeviceVector(ctx, n * n) if want_cov else None
    dse = lsq.DeviceVector(ctx, n) if want_se else None
    df = lsq.DeviceVector(ctx, Jd.m, f) if f is not None else None
    info = np.full(1, -5, dtype=np.int32)
    rc = lsq.lib().lsq_dense_qr_covariance(sv.h, Jd.h, df.ptr if df else None, dcov.ptr if dcov else None,
                                           dse.ptr if dse else None, info.ctypes.data_as(lsq._lib.c_ip))
    return rc, (dcov.get() if want_cov and rc == 0 else None), (dse.get() if want_se and rc == 0 else None), int(info[0])


@pytest.mark.parametrize("m,n,family,env", [(50, 3, "plain", {}), (300, 65, "plain", {}), (500, 130, "plain", {}),
                                            (50, 3, "shuffled-graded", {}),
                                            (300, 65, "shuffled-graded", dict(TWO, LSQ_QR_ALWAYS_PIVOT="1")),
                                            (500, 130, "shuffled-graded", {"LSQ_QR_ONE_STAGE": "1"})])
def test_bits(ctx, monkeypatch, m, n, family, env):
    r = qc.ref(family, m, n)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    Jd, sv = solver_on(ctx, r.A)
    a = sv.dense_qr_covariance(f=r.f)
    assert np.all(np.isfinite(a.cov)) and np.all(np.isfinite(a.stderr))
    assert np.array_equal(a.cov, a.cov.T)
    b = sv.dense_qr_covariance(f=r.f)
    assert np.array_equal(a.cov, b.cov) and np.array_equal(a.stderr, b.stderr)
    lsq.debug_set(serial=1)
    try:
        ser = sv.dense_qr_covariance(f=r.f)
    finally:
        lsq.debug_set(serial=0)
    assert np.array_equal(a.cov, ser.cov) and np.array_equal(a.stderr, ser.stderr)
    # stderr: the same bits with and without d_cov; and sqrt(diag(cov)) to rounding
    rc1, cov1, se1, i1 = raw_call(ctx, sv, Jd, r.f, True, True)
    rc2, _, se2, i2 = raw_call(ctx, sv, Jd, r.f, False, True)
    rc3, cov3, _, i3 = raw_call(ctx, sv, Jd, r.f, True, False)
    assert (rc1, rc2, rc3) == (0, 0, 0) and (i1, i2, i3) == (n, n, n)
    assert np.array_equal(se1, se2) and np.array_equal(se1, a.stderr)
    assert np.array_equal(cov1, cov3) and np.array_equal(cov1.reshape((n, n), order="F"), a.cov)
    # (two sums of at most n non-negative terms in different orders: gamma_n each, halved by the root; s^2 and the root: 4 more)
    assert np.all(np.abs(se1 - np.sqrt(np.diag(a.cov))) <= (2 * n + 8) * ac.UNIT * se1)
    # for_lm = 1 stacks n zero rows: other slab splits, so the rule only
    Jd2, sv2 = solver_on(ctx, r.A, for_lm=True)
    ac.judge("dense qr covariance %s %dx%d for_lm=1" % (family, m, n), device_pieces(r, sv2))
    for o in (sv, sv2, Jd, Jd2):
        o.free()


# ------------------------------------------------------------------------------------------ 4. rank deficiency and reuse
@pytest.mark.parametrize("spoil", ["zero column", "copied column"])
def test_rank_deficient_then_reuse(ctx, spoil):
    m, n, zc = 400, 70, 66                         # (column 66: inside the second 64-block)
    A = ac.dense_operand("plain", m, n, ac.dense_seed(m, n)).J
    bad = A.copy(order="F")
    bad[:, zc] = 0.0 if spoil == "zero column" else bad[:, 2]
    Jd, sv = solver_on(ctx, bad)
    rc, _, _, info = raw_call(ctx, sv, Jd, None, True, True)
    msg = lsq.lib().lsq_last_error().decode()
    print(spoil, "->", rc, info, msg)
    assert rc == ERANK and info == n - 1
    assert "RankDeficientException" in msg and "rank %d" % (n - 1) in msg and "n = %d" % n in msg
    assert sv.info()["qr_rank"] == n - 1
    with pytest.raises(lsq.RankDeficientException) as ec:
        sv.dense_qr_covariance()
    assert ec.value.status == ERANK
    # the same solver on the unspoilt operand: the bits of a fresh solver (nothing stale is read)
    Jd.set_values(A.reshape(-1, order="F"))
    f = np.random.default_rng(5).standard_normal(m)
    again = sv.dense_qr_covariance(f=f)
    Jf, sf = solver_on(ctx, A)
    fresh = sf.dense_qr_covariance(f=f)
    assert np.all(np.isfinite(again.cov)) and np.all(np.isfinite(again.stderr))
    assert np.array_equal(again.cov, fresh.cov) and np.array_equal(again.stderr, fresh.stderr)
    # ... and it still solves
    xs = []
    for solver in (sv, sf):
        dx = lsq.DeviceVector(ctx, n)
        solver.ldiv_(dx, lsq.DeviceVector(ctx, m, f))
        xs.append(dx.get())
    x_ref = ac.qr_fp64_solve(A, f)
    assert np.array_equal(xs[0], xs[1])
    assert np.max(np.abs(xs[0] - x_ref)) <= 1e-11 * np.max(np.abs(x_ref))
    for o in (sv, sf, Jd, Jf):
        o.free()


# ------------------------------------------------------------------------------------------ 5. an exchange gives up
def test_exchange_gives_up_and_the_call_repeats(ctx, monkeypatch):
    m, n = 300, 65
    r = qc.ref("plain", m, n)
    Jd, sv = solver_on(ctx, r.A)
    before = sv.stats()["qr_exchange"]["giveups"]
    monkeypatch.setenv("LSQ_TEST_EXCHANGE_TIMEOUT", "1")
    cov = sv.dense_qr_covariance(f=r.f)
    monkeypatch.delenv("LSQ_TEST_EXCHANGE_TIMEOUT")
    assert sv.stats()["qr_exchange"]["giveups"] == before + 1
    ac.judge("dense qr covariance 300x65 after a give-up", r.pieces("f", cov.cov, cov.stderr, True))
    sv.free()
    Jd.free()


# ------------------------------------------------------------------------------------------ 6. column-scaled dense handle
def test_column_scaled_handle(ctx):
    m, n = 300, 65
    V, f = qc.operand("plain", m, n)
    s = ac.grading(n)
    r = qc.Ref(V * s, f, A_eff=hp.ld(V) * hp.ld(s))          # the handle means V diag(s), unrounded
    Jd = lsq.DeviceMatrix(ctx, V)
    ds = lsq.DeviceVector(ctx, n, s)
    Jd.set_colscale(ds)
    sv = lsq.AllocatedSolver(Jd, lsq.QR(), for_lm=False)
    ac.judge("dense qr covariance colscale 300x65", device_pieces(r, sv))
    sv.free()
    Jd.free()


# ------------------------------------------------------------------------------------------ 7. refusals through the C ABI
def test_refusals(ctx):
    L = lsq.lib()
    m, n = 12, 3
    rng = np.random.default_rng(3)
    A = rng.standard_normal((m, n))
    dense, qr = solver_on(ctx, A)
    out = lsq.DeviceVector(ctx, 64 * 64)
    f = lsq.DeviceVector(ctx, 64)
    import scipy.sparse as sp
    csc = lsq.DeviceMatrix(ctx, sp.csc_matrix(A))
    bd = lsq.DeviceMatrix(ctx, lsq.BlockDiagonal(4, 3, 3, data=lsq.synthetic.blockdiag_inputs(4, 3, 3, 1)))          # 12 x 12
    bb = lsq.DeviceMatrix(ctx, lsq.BorderedBlockDiagonal(2, 6, 1, 1, data=lsq.synthetic.bordered_inputs(2, 6, 1, 1, 1)))   # 12 x 3
    other = lsq.DeviceMatrix(ctx, rng.standard_normal((m, n + 1)))
    square, qr_sq = solver_on(ctx, rng.standard_normal((n, n)) + 3 * np.eye(n))
    wide, qr_wide = solver_on(ctx, rng.standard_normal((2, n)))
    chol = lsq.AllocatedSolver(dense, lsq.Cholesky(), for_lm=True)
    cases = [
        ("both outputs NULL", qr, dense, None, None, None, "both NULL"),
        ("a Cholesky solver", chol, dense, None, out.ptr, None, "needs a QR() solver"),
        ("an LSMR solver", lsq.AllocatedSolver(dense, lsq.LSMR(), for_lm=True), dense, None, out.ptr, None, "needs a QR() solver"),
        ("a BlockQR solver", lsq.AllocatedSolver(bd, lsq.BlockQR(), for_lm=True), bd, None, out.ptr, None, "needs a QR() solver"),
        ("a CSC handle", qr, csc, None, out.ptr, None, "not a dense handle"),
        ("a block-diagonal handle", qr, bd, None, out.ptr, None, "not a dense handle"),
        ("a bordered handle", qr, bb, None, out.ptr, None, "not a dense handle"),
        ("another shape", qr, other, None, out.ptr, None, "allocated for a 12 x 3"),
        ("m < n", qr_wide, wide, None, out.ptr, out.ptr, "needs m >= n"),
        ("m < n with f", qr_wide, wide, f.ptr, None, out.ptr, "needs m >= n"),
        ("m = n with f", qr_sq, square, f.ptr, out.ptr, out.ptr, "needs m > n"),
    ]
    for label, sv, J, pf, pcov, pse, fragment in cases:
        rc = L.lsq_dense_qr_covariance(sv.h, J.h, pf, pcov, pse, None)
        msg = L.lsq_last_error().decode()
        print(label, "->", rc, msg)
        assert rc == EARG, (label, rc)
        assert msg.startswith("lsq_dense_qr_covariance:") and fragment in msg, (label, msg)
    with pytest.raises(lsq.ArgumentError) as ea:                           # ... and as the Python exception
        chol.dense_qr_covariance()
    assert "needs a QR() solver" in str(ea.value)
    for refused in (bd, bb, csc):                                          # (no QR() solver exists on these handles)
        with pytest.raises(lsq.ArgumentError):
            lsq.dense_qr_covariance(refused)
    # lsq_dense_covariance still refuses the QR solver
    rc = L.lsq_dense_covariance(qr.h, dense.h, None, out.ptr, None, None)
    assert rc == EARG and "needs a Cholesky() solver" in L.lsq_last_error().decode()
    # the solvers still work after the refusals; m = n without f is served
    cov = qr.dense_qr_covariance()
    r = qc.Ref(np.asfortranarray(A), np.zeros(m))
    ac.judge("dense qr covariance after refusals", r.pieces("unscaled", cov.cov, cov.stderr, False))
    assert np.all(np.isfinite(qr_sq.dense_qr_covariance().cov))


# ------------------------------------------------------------------------------------------ 8. after a fit
def test_standard_errors_after_a_dense_fit(ctx):
    """a exp(-k t) + c with 1 % noise (the decay of tests/test_j_gpu_dense_covariance.py, restated), Dogleg(QR()), then the
    covariance at the solution with the residual, against the longdouble reference on the host copy of the final Jacobian."""
    m, n = 40, 3
    t = np.linspace(0.0, 4.0, m)
    rng = np.random.default_rng(42)
    data = 1.5 * np.exp(-0.8 * t) + 0.3 + 0.01 * rng.standard_normal(m)

    def f_(out, x):
        out[:] = x[0] * np.exp(-x[1] * t) + x[2] - data

    def g_(J, x):
        e = np.exp(-x[1] * t)
        J[:, 0], J[:, 1], J[:, 2] = e, -x[0] * t * e, 1.0

    nls = lsq.LeastSquaresProblem(x=np.array([1.0, 1.0, 0.0]), y=np.zeros(m), f_=f_, g_=g_, J=np.zeros((m, n), order="F"))
    res = lsq.optimize_(nls, lsq.Dogleg(lsq.QR()), ctx=ctx)
    assert res.converged
    x = np.array(res.minimizer)
    Jf, fcur = np.zeros((m, n), order="F"), np.zeros(m)
    g_(Jf, x)
    f_(fcur, x)
    cov = lsq.dense_qr_covariance(lsq.DeviceMatrix(ctx, Jf), f=fcur)
    print("fit x %s stderr %s" % (x, cov.stderr))
    ac.judge("dense qr covariance after a fit", qc.Ref(Jf, fcur).pieces("f", cov.cov, cov.stderr, True))
    assert np.all(cov.stderr < 0.1)                                        # the parameters ARE determined (noise 1%)


# ------------------------------------------------------------------------------------------ 9. where it matters
def test_six_decades_where_the_normal_equations_fail(ctx):
    """ill6 at 300 x 65, cond(J) = 1e6: the QR() covariance passes the rule; lsq_dense_covariance, which factors J'J
    (cond 1e12), either reports PosDefException or misses the same bound."""
    m, n = 300, 65
    r = qc.ref("ill6", m, n)
    Jd, sv = solver_on(ctx, r.A)
    cov = sv.dense_qr_covariance(f=r.f)
    ac.judge("dense qr covariance ill6 300x65", r.pieces("f", cov.cov, cov.stderr, True))
    chol = lsq.AllocatedSolver(Jd, lsq.Cholesky(), for_lm=True)
    try:
        c2 = chol.dense_covariance(f=r.f)
    except lsq.PosDefException as e:
        print("lsq_dense_covariance on ill6 300x65:", e)
    else:
        pieces = r.pieces("f", c2.cov, c2.stderr, True)
        print("lsq_dense_covariance on ill6 300x65:", [(p[0], "%.3e" % p[1], "bound %.3e" % ac.bound(p[2], p[3])) for p in pieces])
        assert not all(ac.accepted(d, e_ref, k) for _, d, e_ref, k in pieces)
    for o in (sv, chol, Jd):
        o.free()
