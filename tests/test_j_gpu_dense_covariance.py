"""Parameter covariance of a plain dense Jacobian on the device (lsq_dense_covariance, lsq_cov_dense.hip: the MFMA SYRK and
blocked Cholesky of the solves, the explicit inverse X = inv(U) of the certificates, then k_cov_xxt: inv(J'J) = X X' per
64 x 64 upper tile, and k_cov_stderr).  Runs behind the accuracy tier and takes its operands, metrics and rule unchanged
(tests/accuracy_common.py, tests/hp_reference.py):
    H        hp.inv_gram(A) in numpy.longdouble, times ac.s2_of(f, m - n) with a residual
    e_ref    numpy.linalg.inv(A.T @ A) in fp64 (times the fp64 variance), as tests/test_h_gpu_accuracy.py
    rule     ac.judge(ac.cov_pieces(.., k = n)): e_dev <= 16 max(e_ref, min(max(16, n), 64) 2^-53), covariance and stderr
tests/test_dense_covariance_host.py shows on the CPU that the fp64 stand-in of the device algorithm (ac.standin_inv) and numpy
both stay inside that rule on the eight shapes: closest ill 50 x 3 (e 4.5e-11, bound 3.3e-10), the non-ill families below
3.6e-15 against bounds >= 2.8e-14 -- a correct kernel has 7 x of room, a masking mistake in a diagonal block has none.

Two places where this file cannot follow the letter of its specification, and follows its sense:
  * hp.inv_gram ignores `colscale` for a dense operand (only the bordered branch applies it), so the column-scaled case forms
    the effective Jacobian V diag(s) in longdouble itself and hands THAT to hp.inv_gram -- the unrounded operand, as
    ac.bd_effective does for the block handles.
  * every problem of tests/problems.py is square (m = n: no residual variance, sum(f.^2) / (m - n)) or, the factor model,
    rank-deficient at its solution.  The end-to-end case therefore fits a three-parameter decay with m = 40 > n, defined
    here, with the residual; a square problem of tests/problems.py (helical valley) is fitted as well and checked without one.
"""
import functools

import numpy as np
import pytest

import accuracy_common as ac
import hp_reference as hp
import problems as P
from gpu_common import lsq

pytestmark = pytest.mark.gpu

EARG, ENOTPD = lsq._lib.EARG, lsq._lib.ENOTPD

# one tile (n = 1, 3, 31: the one-workgroup factorisation; 64: the blocked one), a ragged second tile, three ragged tiles,
# four, and six tiles of which the last has one column
SHAPES = [(40, 1), (50, 3), (90, 31), (200, 64), (300, 65), (500, 130), (700, 200), (1000, 321)]
CASES = [(m, n, fam) for (m, n) in SHAPES for fam in ac.FAMILIES if not (fam == "graded" and n == 1)]   # (ac.grading: k - 1 = 0)


class Ref:
    def __init__(self, A, f):
        m, n = A.shape
        self.A, self.f, self.m, self.n = A, f, m, n
        self.H = hp.inv_gram(A)                                   # longdouble
        self.R = np.linalg.inv(A.T @ A)                           # fp64: e_ref
        self.s2_hp = ac.s2_of(f, m - n) if m > n else None
        self.s2 = float(f @ f) / (m - n) if m > n else None

    def pieces(self, name, cov, with_f):
        s_hp, s64 = (self.s2_hp, self.s2) if with_f else (hp.LD(1), 1.0)
        return ac.cov_pieces(name, cov.cov, cov.stderr, s64 * self.R, self.H * s_hp, self.n)


@functools.lru_cache(maxsize=8)
def ref(family, m, n):
    op = ac.dense_operand(family, m, n, ac.dense_seed(m, n))
    return Ref(op.J, op.y)            # (y: standard normal, scaled with the operand in far+ / far-: the residual of the case)


def solver_on(ctx, A, for_lm=True):
    Jd = lsq.DeviceMatrix(ctx, A)
    return Jd, lsq.AllocatedSolver(Jd, lsq.Cholesky(), for_lm=for_lm)


def blocked_shape(m, n):
    """The operands lsq_ldiv_damped, and with it lsq_dense_covariance, sends to the blocked factorisation."""
    return n >= 32 or (n >= 2 and m * n >= 20000)


# ------------------------------------------------------------------------------------------ 1. accuracy
@pytest.mark.parametrize("m,n,family", CASES)
def test_accuracy(ctx, m, n, family):
    r = ref(family, m, n)
    Jd, sv = solver_on(ctx, r.A)
    pieces = []
    for with_f in (False, True):
        cov = sv.dense_covariance(f=r.f if with_f else None)
        assert cov.n == n and cov.cov.shape == (n, n) and cov.stderr.shape == (n,)
        pieces += r.pieces("f" if with_f else "unscaled", cov, with_f)
    path = sv.info()["chol_path"]
    print("PATH dense covariance %dx%d %s | %s" % (m, n, family, path))
    assert path in (("blocked", "blocked-one-launch") if blocked_shape(m, n) else ("one-workgroup",))
    ac.judge("dense covariance %s %dx%d" % (family, m, n), pieces)
    sv.free()
    Jd.free()


# ------------------------------------------------------------------------------------------ 2. triangles and bits
def raw_call(ctx, sv, Jd, f, want_cov, want_se):
    """lsq_dense_covariance through the C ABI: (rc, cov or None, stderr or None, h_info)."""
    n = Jd.n
    dcov = lsq.DeviceVector(ctx, n * n) if want_cov else None
    dse = lsq.DeviceVector(ctx, n) if want_se else None
    df = lsq.DeviceVector(ctx, Jd.m, f) if f is not None else None
    info = np.full(1, -5, dtype=np.int32)
    rc = lsq.lib().lsq_dense_covariance(sv.h, Jd.h, df.ptr if df else None, dcov.ptr if dcov else None,
                                        dse.ptr if dse else None, info.ctypes.data_as(lsq._lib.c_ip))
    return rc, (dcov.get() if want_cov and rc == 0 else None), (dse.get() if want_se and rc == 0 else None), int(info[0])


@pytest.mark.parametrize("m,n", [(50, 3), (300, 65), (500, 130)])
def test_triangles_and_bits(ctx, m, n):
    r = ref("plain", m, n)
    Jd, sv = solver_on(ctx, r.A)
    a = sv.dense_covariance(f=r.f)
    assert np.all(np.isfinite(a.cov)) and np.all(np.isfinite(a.stderr))
    assert np.array_equal(a.cov, a.cov.T)
    b = sv.dense_covariance(f=r.f)
    assert np.array_equal(a.cov, b.cov) and np.array_equal(a.stderr, b.stderr)
    lsq.debug_set(serial=1)
    try:
        ser = sv.dense_covariance(f=r.f)
    finally:
        lsq.debug_set(serial=0)
    assert np.array_equal(a.cov, ser.cov) and np.array_equal(a.stderr, ser.stderr)
    Jd2, sv2 = solver_on(ctx, r.A, for_lm=False)
    d = sv2.dense_covariance(f=r.f)
    assert np.array_equal(a.cov, d.cov) and np.array_equal(a.stderr, d.stderr)
    # stderr: the same bits with and without d_cov; and sqrt(diag(cov)) to rounding
    rc1, cov1, se1, _ = raw_call(ctx, sv, Jd, r.f, True, True)
    rc2, _, se2, _ = raw_call(ctx, sv, Jd, r.f, False, True)
    rc3, cov3, _, _ = raw_call(ctx, sv, Jd, r.f, True, False)
    assert (rc1, rc2, rc3) == (0, 0, 0)
    assert np.array_equal(se1, se2) and np.array_equal(se1, a.stderr)
    assert np.array_equal(cov1, cov3) and np.array_equal(cov1.reshape((n, n), order="F"), a.cov)
    # (two sums of at most n non-negative terms in different orders: gamma_n each, halved by the root; s^2 and the root: 4 more)
    assert np.all(np.abs(se1 - np.sqrt(np.diag(a.cov))) <= (2 * n + 8) * ac.UNIT * se1)
    for o in (sv, sv2, Jd, Jd2):
        o.free()


# ------------------------------------------------------------------------------------------ 3. both factorisations at 1000 x 321
@pytest.mark.parametrize("env,expect", [({}, "blocked-one-launch"), ({"LSQ_CHOL_PANELS": "1"}, "blocked")])
def test_both_factorisations(ctx, monkeypatch, env, expect):
    m, n = 1000, 321
    r = ref("plain", m, n)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    Jd, sv = solver_on(ctx, r.A)
    cov = sv.dense_covariance(f=r.f)
    assert sv.info()["chol_path"] == expect
    ac.judge("dense covariance 1000x321 %s" % expect, r.pieces("f", cov, True))
    sv.free()
    Jd.free()


def test_one_launch_gives_up_and_panels_take_over(ctx, monkeypatch):
    m, n = 1000, 321
    r = ref("plain", m, n)
    Jd, sv = solver_on(ctx, r.A)
    before = sv.stats()["chol_one_launch"]["giveups"]
    monkeypatch.setenv("LSQ_TEST_EXCHANGE_TIMEOUT", "1")
    cov = sv.dense_covariance(f=r.f)
    monkeypatch.delenv("LSQ_TEST_EXCHANGE_TIMEOUT")
    assert sv.stats()["chol_one_launch"]["giveups"] == before + 1
    assert sv.info()["chol_path"] == "blocked"
    ac.judge("dense covariance 1000x321 after a give-up", r.pieces("f", cov, True))
    sv.free()
    Jd.free()


# ------------------------------------------------------------------------------------------ 4. column-scaled dense handle
def test_column_scaled_handle(ctx):
    m, n = 300, 65
    V = ac.dense_operand("plain", m, n, ac.dense_seed(m, n)).J
    s = ac.grading(n)
    H = hp.inv_gram(hp.ld(V) * hp.ld(s))          # the handle means V diag(s); hp.inv_gram(V, colscale=s) would ignore s here
    A64 = V * s
    R = np.linalg.inv(A64.T @ A64)
    Jd = lsq.DeviceMatrix(ctx, V)
    ds = lsq.DeviceVector(ctx, n, s)
    Jd.set_colscale(ds)
    sv = lsq.AllocatedSolver(Jd, lsq.Cholesky(), for_lm=True)
    cov = sv.dense_covariance()
    ac.judge("dense covariance colscale 300x65", ac.cov_pieces("unscaled", cov.cov, cov.stderr, R, H, n))
    sv.free()
    Jd.free()


# ------------------------------------------------------------------------------------------ 5. failure and reuse
def test_not_positive_definite_then_reuse(ctx):
    m, n, zc = 400, 70, 66                         # (column 66: inside the second 64-block)
    A = ac.dense_operand("plain", m, n, ac.dense_seed(m, n)).J
    bad = A.copy(order="F")
    bad[:, zc] = 0.0
    msg = "PosDefException: matrix is not positive definite; Cholesky failed at %d" % (zc + 1)
    Jd, sv = solver_on(ctx, bad)
    rc, _, _, info = raw_call(ctx, sv, Jd, None, True, True)
    assert rc == ENOTPD and info == zc + 1
    assert lsq.lib().lsq_last_error().decode() == msg
    with pytest.raises(lsq.PosDefException) as ec:
        sv.dense_covariance()
    Jz, sz = solver_on(ctx, bad)                   # the exception lsq_ldiv_damped raises for the same operand (no damping added)
    with pytest.raises(lsq.PosDefException) as es:
        sz.ldiv_(lsq.DeviceVector(ctx, n), lsq.DeviceVector(ctx, m, np.ones(m)), lsq.DeviceVector(ctx, n))
    assert ec.value.status == es.value.status == ENOTPD
    assert str(ec.value) == str(es.value) == msg
    # the same solver on the unspoilt operand: the bits of a fresh solver (nothing stale is read)
    Jd.set_values(A.reshape(-1, order="F"))
    f = np.random.default_rng(5).standard_normal(m)
    again = sv.dense_covariance(f=f)
    Jf, sf = solver_on(ctx, A)
    fresh = sf.dense_covariance(f=f)
    assert np.all(np.isfinite(again.cov)) and np.all(np.isfinite(again.stderr))
    assert np.array_equal(again.cov, fresh.cov) and np.array_equal(again.stderr, fresh.stderr)
    # ... and it still solves
    damp = 0.05 + np.random.default_rng(6).random(n)
    xs = []
    for solver, J in ((sv, Jd), (sf, Jf)):
        dx = lsq.DeviceVector(ctx, n)
        solver.ldiv_(dx, lsq.DeviceVector(ctx, m, f), lsq.DeviceVector(ctx, n, damp))
        xs.append(dx.get())
    x_ref = np.linalg.solve(A.T @ A + np.diag(damp), A.T @ f)
    assert np.max(np.abs(xs[0] - xs[1])) <= 1e-12 * np.max(np.abs(xs[1]))
    assert np.max(np.abs(xs[0] - x_ref)) <= 1e-9 * np.max(np.abs(x_ref))
    for o in (sv, sz, sf, Jd, Jz, Jf):
        o.free()


# ------------------------------------------------------------------------------------------ 6. refusals through the C ABI
def test_refusals(ctx):
    L = lsq.lib()
    m, n = 12, 3
    rng = np.random.default_rng(3)
    A = rng.standard_normal((m, n))
    dense, chol = solver_on(ctx, A)
    out = lsq.DeviceVector(ctx, 64 * 64)
    f = lsq.DeviceVector(ctx, 64)
    import scipy.sparse as sp
    csc = lsq.DeviceMatrix(ctx, sp.csc_matrix(A))
    bd_host = lsq.BlockDiagonal(4, 3, 3, data=lsq.synthetic.blockdiag_inputs(4, 3, 3, 1))                 # 12 x 12
    bd = lsq.DeviceMatrix(ctx, bd_host)
    bb = lsq.DeviceMatrix(ctx, lsq.BorderedBlockDiagonal(2, 6, 1, 1, data=lsq.synthetic.bordered_inputs(2, 6, 1, 1, 1)))   # 12 x 3
    op = lsq.DeviceOperator(ctx, m, n, lambda trans, x, o: None, lambda o: None)
    other = lsq.DeviceMatrix(ctx, rng.standard_normal((m, n + 1)))
    square, chol_sq = solver_on(ctx, rng.standard_normal((n, n)) + 3 * np.eye(n))
    wide, chol_wide = solver_on(ctx, rng.standard_normal((2, n)))
    cases = [
        ("both outputs NULL", chol, dense, None, None, None),
        ("a QR solver", lsq.AllocatedSolver(dense, lsq.QR(), for_lm=True), dense, None, out.ptr, None),
        ("an LSMR solver", lsq.AllocatedSolver(dense, lsq.LSMR(), for_lm=True), dense, None, out.ptr, None),
        ("a block-diagonal solver and handle", lsq.AllocatedSolver(bd, lsq.Cholesky(), for_lm=True), bd, None, out.ptr, None),
        ("a bordered solver and handle", lsq.AllocatedSolver(bb, lsq.Cholesky(), for_lm=True), bb, None, out.ptr, None),
        ("a CSC handle", chol, csc, None, out.ptr, None),
        ("a block-diagonal handle", chol, bd, None, out.ptr, None),
        ("a bordered handle", chol, bb, None, out.ptr, None),
        ("an operator handle", chol, op, None, out.ptr, None),
        ("another shape", chol, other, None, out.ptr, None),
        ("m = n with f", chol_sq, square, f.ptr, out.ptr, out.ptr),
        ("m < n with f", chol_wide, wide, f.ptr, None, out.ptr),
    ]
    for label, sv, J, pf, pcov, pse in cases:
        rc = L.lsq_dense_covariance(sv.h, J.h, pf, pcov, pse, None)
        msg = L.lsq_last_error().decode()
        print(label, "->", rc, msg)
        assert rc == EARG, (label, rc)
        assert msg.startswith("lsq_dense_covariance:"), (label, msg)
    for refused in (bd, bb, csc):                                          # ... and as the Python exception
        with pytest.raises(lsq.ArgumentError):
            lsq.dense_covariance(refused)
    # the solvers still work after the refusals; m = n without f is served
    cov = chol.dense_covariance()
    H = hp.inv_gram(A)
    ac.judge("dense covariance after refusals", ac.cov_pieces("unscaled", cov.cov, cov.stderr, np.linalg.inv(A.T @ A), H, n))
    assert np.all(np.isfinite(chol_sq.dense_covariance().cov))


# ------------------------------------------------------------------------------------------ 7. after a fit
def test_standard_errors_after_a_dense_fit(ctx):
    """a exp(-k t) + c with 1 % noise, LevenbergMarquardt(Cholesky()), then the covariance at the solution against the
    longdouble reference on the host copy of the final Jacobian, by the rule."""
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
    r = lsq.optimize_(nls, lsq.LevenbergMarquardt(lsq.Cholesky()), ctx=ctx)
    assert r.converged
    x = np.array(r.minimizer)
    Jf, fcur = np.zeros((m, n), order="F"), np.zeros(m)
    g_(Jf, x)
    f_(fcur, x)
    cov = lsq.dense_covariance(lsq.DeviceMatrix(ctx, Jf), f=fcur)
    rf = Ref(Jf, fcur)
    print("fit x %s stderr %s" % (x, cov.stderr))
    ac.judge("dense covariance after a fit", rf.pieces("f", cov, True))
    assert np.all(cov.stderr < 0.1)                                        # the parameters ARE determined (noise 1%)

    # a problem of tests/problems.py: square, so no residual variance -- the unscaled inv(J'J) at its solution
    name, f, g, x0 = P.helical_valley()[:4]
    k = len(x0)
    nls = lsq.LeastSquaresProblem(x=x0.copy(), y=np.zeros(k), f_=f, g_=g, J=np.zeros((k, k), order="F"))
    r = lsq.optimize_(nls, lsq.LevenbergMarquardt(lsq.Cholesky()), ctx=ctx)
    assert r.converged
    Jh = np.zeros((k, k), order="F")
    g(Jh, np.array(r.minimizer))
    cov = lsq.dense_covariance(lsq.DeviceMatrix(ctx, Jh))
    ac.judge("dense covariance helical valley", Ref(Jh, np.zeros(k)).pieces("unscaled", cov, False))
