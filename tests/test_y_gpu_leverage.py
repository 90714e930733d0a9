"""Leverages and prediction variances on the device (lsq_leverage.hip: k_lev_tall, k_lev_diag, k_bd_lev behind
lsq_dense_qr_leverage and lsq_solver_leverage).  Operands, the longdouble reference, the fp64 e_ref and the numpy twins are in
tests/leverage_common.py; the rule is the accuracy tier's, unchanged:
    ac.judge(pieces with k = n, nb per block): e_dev <= 16 max(e_ref, min(max(16, k), 64) 2^-53),  e(q) = max_i |q_i - q_hp,i| / q_hp,i
tests/test_leverage_host.py shows on the CPU that the twin of the device's algebra stays inside it on every dense case here, that
planted mistakes do not, and that on the block handle one Cholesky of J_b'J_b does not on the `ill` family, which is why
k_bd_lev is a CholeskyQR2."""
import ctypes as C

import numpy as np
import pytest

import accuracy_common as ac
import hp_reference as hp
import leverage_common as lc
import qr_cov_common as qc
from gpu_common import lsq
from test_n_gpu_dense_qr_covariance import PATH_SWITCHES, PIVOTED

pytestmark = pytest.mark.gpu

EARG, ERANK = lsq._lib.EARG, lsq._lib.ERANK


def solver_on(ctx, A, for_lm=False):
    Jd = lsq.DeviceMatrix(ctx, A)
    return Jd, lsq.AllocatedSolver(Jd, lsq.QR(), for_lm=for_lm)


def raw(ctx, sv, Jd, f=None, A=None, lda=None, want=("q", "se", "t", "cook", "s2")):
    """lsq_dense_qr_leverage through the C ABI.  A: p x n host rows, uploaded with leading dimension lda (default p), the
    padding rows NaN.  Returns (rc, dict of the outputs asked for, h_info)."""
    rows = Jd.m
    dA, p, ld = None, 0, 0
    if A is not None:
        p = A.shape[0]
        ld = p if lda is None else lda
        buf = np.full((ld, A.shape[1]), np.nan, order="F")
        buf[:p] = A
        dA = lsq.DeviceVector(ctx, buf.size, buf.reshape(-1, order="F"))
        rows = p
    df = lsq.DeviceVector(ctx, Jd.m, f) if f is not None else None
    out = {k: lsq.DeviceVector(ctx, rows, np.full(rows, -7.0)) for k in want if k != "s2"}
    s2 = C.c_double(-7.0)
    info = np.full(1, -5, dtype=np.int32)
    ptr = lambda k: out[k].ptr if k in out else None
    rc = lsq.lib().lsq_dense_qr_leverage(sv.h, Jd.h, dA.ptr if dA else None, p, ld, df.ptr if df else None, ptr("q"), ptr("se"),
                                         ptr("t"), ptr("cook"), C.byref(s2) if "s2" in want else None,
                                         info.ctypes.data_as(lsq._lib.c_ip))
    res = {k: v.get() for k, v in out.items()} if rc == 0 else {}
    if rc == 0 and "s2" in want:
        res["s2"] = s2.value
    return rc, res, int(info[0])


def device_pieces(r, sv, name=""):
    """Both calls (without and with the residual) on J's own rows, as pieces for ac.judge."""
    a = sv.dense_qr_leverage()
    b = sv.dense_qr_leverage(f=r.f)
    assert a.q.shape == (r.m,) and a.se is None and a.rank == r.n and b.rank == r.n
    assert np.array_equal(a.q, b.q)
    return lc.pieces(name + "unscaled", a.q, r) + lc.pieces(name + "f", b.q, r, True, b.se)


# ------------------------------------------------------------------------------------------ 1. accuracy
@pytest.mark.parametrize("m,n,family", lc.CASES)
def test_accuracy(ctx, m, n, family):
    r = lc.ref(family, m, n)
    Jd, sv = solver_on(ctx, r.J)
    pieces = device_pieces(r, sv)
    info = sv.info()
    print("PATH dense qr leverage %dx%d %s | %s %s rank %s" % (m, n, family, info["qr_path"], info["qr_panel"], info["qr_rank"]))
    ac.judge("dense qr leverage %s %dx%d" % (family, m, n), pieces)
    sv.free()
    Jd.free()


# ------------------------------------------------------------------------------------------ 2. every factorisation path
@pytest.mark.parametrize("switch", list(PATH_SWITCHES))
@pytest.mark.parametrize("family", ["plain", "shuffled-graded"])
@pytest.mark.parametrize("m,n", [(300, 65), (500, 130)])
def test_every_path(ctx, monkeypatch, m, n, family, switch):
    env, expect = PATH_SWITCHES[switch]
    r = lc.ref(family, m, n)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    Jd, sv = solver_on(ctx, r.J, for_lm=True)
    pieces = device_pieces(r, sv)
    q = sv.dense_qr_leverage().q
    info = sv.info()
    what = "%s %dx%d %s for_lm=1" % (switch, m, n, family)
    print("PATH dense qr leverage %s | %s %s rank %s" % (what, info["qr_path"], info["qr_panel"], info["qr_rank"]))
    for key, want in expect.items():
        assert info[key] == want, (what, key, info)
    ac.judge("dense qr leverage " + what, pieces)
    if family == "shuffled-graded" and switch in PIVOTED:
        # the factor was pivoted (graded columns, shuffled): leaving the permutation out is far from what the device returns
        wrong = lc.twin_dense(r.J, mistake="no-permutation")
        assert lc.lev_err(wrong, r.q_hp) > 1e3 and lc.lev_err(q, wrong) > 0.5
    sv.free()
    Jd.free()


# ------------------------------------------------------------------------------------------ 3. kernel edges, new rows
@pytest.mark.parametrize("n", [1, 3, 64, 65, 130])
def test_new_rows_edges(ctx, n):
    """p = 1, 63, 64, 65, 129 rows (one lane of a slab, a slab less one, a full slab, one row into the second, one into the
    third) against n = 1, 3, 64, 65, 130 columns (one ragged tile, a full one, one column into the second, into the third), with
    lda = p and lda = p + 3 (NaN in the padding rows)."""
    m = n + 70
    J, f = qc.operand("plain", m, n)
    Jd, sv = solver_on(ctx, J)
    rng = np.random.default_rng(100 + n)
    for p in (1, 63, 64, 65, 129):
        A = np.asfortranarray(rng.standard_normal((p, n)) / np.sqrt(m))
        r = lc.Ref(J, f, A=A)
        rc, tight, rank = raw(ctx, sv, Jd, f=f, A=A, want=("q", "se", "s2"))
        assert rc == 0 and rank == n
        rc, padded, _ = raw(ctx, sv, Jd, f=f, A=A, lda=p + 3, want=("q", "se", "s2"))
        assert rc == 0
        assert np.all(np.isfinite(tight["q"])) and np.array_equal(tight["q"], padded["q"]) and np.array_equal(tight["se"], padded["se"])
        assert tight["s2"] == padded["s2"]
        ac.judge("dense qr leverage new rows p=%d n=%d" % (p, n), lc.pieces("rows", tight["q"], r, True, tight["se"]))
        se_t, _, _ = lc.diag_twin(tight["q"], np.zeros(p), tight["s2"], n)
        assert np.array_equal(tight["se"], se_t)
        py = sv.dense_qr_leverage(f=f, A=A)
        assert np.array_equal(py.q, tight["q"]) and np.array_equal(py.se, tight["se"]) and py.studentized is None
    # A = J: the bits of d_A = NULL; rows [a, b) alone: the bits they have inside the full call
    own = sv.dense_qr_leverage().q
    rc, same, _ = raw(ctx, sv, Jd, A=J, want=("q",))
    assert rc == 0 and np.array_equal(same["q"], own)
    for a, b in ((0, 1), (60, 70), (64, m), (m - 1, m)):
        rc, part, _ = raw(ctx, sv, Jd, A=np.asfortranarray(J[a:b]), lda=(b - a) + 3, want=("q",))
        assert rc == 0 and np.array_equal(part["q"], own[a:b]), (n, a, b)
    sv.free()
    Jd.free()


# ------------------------------------------------------------------------------------------ 4. bits
@pytest.mark.parametrize("m,n,family,env", [(50, 3, "plain", {}), (500, 130, "plain", {}),
                                            (300, 65, "shuffled-graded", {"LSQ_QR_TWO_STAGE": "1", "LSQ_QR_ALWAYS_PIVOT": "1"}),
                                            (500, 130, "shuffled-graded", {"LSQ_QR_ONE_STAGE": "1"})])
def test_bits(ctx, monkeypatch, m, n, family, env):
    r = lc.ref(family, m, n)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    Jd, sv = solver_on(ctx, r.J)
    keys = ("q", "se", "t", "cook", "s2")

    def same(x, y):
        return all(np.array_equal(x[k], y[k]) for k in keys)

    rc, a, _ = raw(ctx, sv, Jd, f=r.f)
    assert rc == 0 and all(np.all(np.isfinite(a[k])) for k in keys)
    rc, b, _ = raw(ctx, sv, Jd, f=r.f)
    assert rc == 0 and same(a, b)
    lsq.debug_set(serial=1)
    try:
        rc, ser, _ = raw(ctx, sv, Jd, f=r.f)
    finally:
        lsq.debug_set(serial=0)
    assert rc == 0 and same(a, ser)
    lsq.debug_set(launch_jitter_us=200)
    try:
        rc, jit, _ = raw(ctx, sv, Jd, f=r.f)
    finally:
        lsq.debug_set(launch_jitter_us=0)
    assert rc == 0 and same(a, jit)
    Jd2, sv2 = solver_on(ctx, r.J)
    rc, other, _ = raw(ctx, sv2, Jd2, f=r.f)
    assert rc == 0 and same(a, other)
    # the derived outputs without d_q (the solver's own buffer) and q alone: the same bits
    rc, noq, _ = raw(ctx, sv, Jd, f=r.f, want=("se", "t", "cook"))
    assert rc == 0 and all(np.array_equal(noq[k], a[k]) for k in ("se", "t", "cook"))
    rc, qonly, _ = raw(ctx, sv, Jd, want=("q",))
    assert rc == 0 and np.array_equal(qonly["q"], a["q"])
    for o in (sv, sv2, Jd, Jd2):
        o.free()


def test_solve_after_leverage_and_covariance_in_either_order(ctx):
    m, n = 500, 130
    r = lc.ref("plain", m, n)
    y = lsq.DeviceVector(ctx, m, r.f)

    def solve(sv):
        dx = lsq.DeviceVector(ctx, n)
        sv.ldiv_(dx, y)
        return dx.get()

    Jd, plain = solver_on(ctx, r.J)
    x0 = solve(plain)
    cov0 = plain.dense_qr_covariance(f=r.f)
    Jd1, sv1 = solver_on(ctx, r.J)
    lev1 = sv1.dense_qr_leverage(f=r.f)
    assert np.array_equal(solve(sv1), x0)                       # a solve after a leverage call: the bits of a solve without one
    cov1 = sv1.dense_qr_covariance(f=r.f)                       # leverage, then covariance
    assert np.array_equal(cov1.cov, cov0.cov) and np.array_equal(cov1.stderr, cov0.stderr)
    lev0 = plain.dense_qr_leverage(f=r.f)                       # covariance, then leverage
    for k in ("q", "se", "studentized", "cook"):
        assert np.array_equal(getattr(lev0, k), getattr(lev1, k)), k
    assert lev0.s2 == lev1.s2 and np.array_equal(solve(plain), x0)
    for o in (plain, sv1, Jd, Jd1):
        o.free()


# ------------------------------------------------------------------------------------------ 5. column-scaled handle
def test_column_scaled_handle(ctx):
    m, n = 300, 65
    V, f = qc.operand("plain", m, n)
    s = ac.grading(n)
    r = lc.Ref(np.asfortranarray(V * s), f, J_eff=hp.ld(V) * hp.ld(s))      # the handle means V diag(s), unrounded
    Jd = lsq.DeviceMatrix(ctx, V)
    ds = lsq.DeviceVector(ctx, n, s)
    Jd.set_colscale(ds)
    sv = lsq.AllocatedSolver(Jd, lsq.QR(), for_lm=False)
    ac.judge("dense qr leverage colscale 300x65", device_pieces(r, sv))
    # new rows are rows of J S already
    A = np.asfortranarray((V * s)[:40])
    got = sv.dense_qr_leverage(A=A)
    ac.judge("dense qr leverage colscale new rows", lc.pieces("rows", got.q, lc.Ref(r.J, f, A=A, J_eff=hp.ld(V) * hp.ld(s))))
    sv.free()
    Jd.free()


# ------------------------------------------------------------------------------------------ 6. k_lev_diag, bit for bit
@pytest.mark.parametrize("m", [255, 256, 257, 513])
def test_diag_kernel_bits(ctx, m):
    """The three derived outputs from the device's own q and s2 and the numpy twin: equal bits.  m around one workgroup of 256
    and one row past a full grid of two; row 7 is the only nonzero of column 1, so h_7 rounds to 1 (or to a neighbour) and
    t_7, cook_7 are whatever IEEE arithmetic gives -- nothing is clamped."""
    n = 3
    J, f = qc.operand("plain", m, n)
    J = J.copy(order="F")
    J[:, 1] = 0.0
    J[7, 1] = 1.0
    Jd, sv = solver_on(ctx, J)
    rc, d, rank = raw(ctx, sv, Jd, f=f)
    assert rc == 0 and rank == n
    assert abs(d["q"][7] - 1.0) <= 64 * ac.UNIT
    assert d["s2"] == sv.dense_qr_leverage(f=f).s2
    se, t, cook = lc.diag_twin(d["q"], f, d["s2"], n)
    print("h_7 - 1 = %.3e, t_7 = %r, cook_7 = %r" % (d["q"][7] - 1.0, d["t"][7], d["cook"][7]))
    assert np.array_equal(d["se"], se)
    assert np.array_equal(d["t"], t, equal_nan=True) and np.array_equal(d["cook"], cook, equal_nan=True)
    assert np.all(np.isfinite(np.delete(d["t"], 7))) and np.all(np.isfinite(np.delete(d["cook"], 7)))
    sv.free()
    Jd.free()


def test_diag_kernel_one_row(ctx):
    """m = 1 leaves no degree of freedom for a variance, so the one-row launch of k_lev_diag is a single new row: se alone."""
    m, n = 40, 3
    J, f = qc.operand("plain", m, n)
    Jd, sv = solver_on(ctx, J)
    A = np.asfortranarray(J[5:6])
    rc, d, _ = raw(ctx, sv, Jd, f=f, A=A, want=("q", "se", "s2"))
    assert rc == 0
    assert np.array_equal(d["se"], lc.diag_twin(d["q"], np.zeros(1), d["s2"], n)[0])
    assert np.array_equal(d["q"], sv.dense_qr_leverage().q[5:6])


# ------------------------------------------------------------------------------------------ 7. rank deficiency and reuse
def test_rank_deficient_then_reuse(ctx):
    m, n, zc = 400, 70, 66
    A = ac.dense_operand("plain", m, n, ac.dense_seed(m, n)).J
    bad = A.copy(order="F")
    bad[:, zc] = bad[:, 2]
    Jd, sv = solver_on(ctx, bad)
    rc, _, info = raw(ctx, sv, Jd, want=("q",))
    msg = lsq.lib().lsq_last_error().decode()
    print("copied column ->", rc, info, msg)
    assert rc == ERANK and info == n - 1
    assert "RankDeficientException" in msg and "rank %d" % (n - 1) in msg and "n = %d" % n in msg
    with pytest.raises(lsq.RankDeficientException) as ec:
        sv.dense_qr_leverage()
    assert ec.value.status == ERANK
    Jd.set_values(A.reshape(-1, order="F"))
    f = np.random.default_rng(5).standard_normal(m)
    again = sv.dense_qr_leverage(f=f)
    Jf, sf = solver_on(ctx, A)
    fresh = sf.dense_qr_leverage(f=f)
    for k in ("q", "se", "studentized", "cook"):
        assert np.all(np.isfinite(getattr(again, k))) and np.array_equal(getattr(again, k), getattr(fresh, k)), k
    for o in (sv, sf, Jd, Jf):
        o.free()


# ------------------------------------------------------------------------------------------ 8. refusals through the C ABI
def test_refusals(ctx):
    L = lsq.lib()
    m, n = 12, 3
    rng = np.random.default_rng(3)
    A = rng.standard_normal((m, n))
    dense, qr = solver_on(ctx, A)
    out = lsq.DeviceVector(ctx, 64)
    f = lsq.DeviceVector(ctx, 64)
    rows = lsq.DeviceVector(ctx, 64)
    import scipy.sparse as sp
    csc = lsq.DeviceMatrix(ctx, sp.csc_matrix(A))
    bd = lsq.DeviceMatrix(ctx, lsq.BlockDiagonal(4, 3, 3, data=lsq.synthetic.blockdiag_inputs(4, 3, 3, 1)))          # 12 x 12
    bb = lsq.DeviceMatrix(ctx, lsq.BorderedBlockDiagonal(2, 6, 1, 1, data=lsq.synthetic.bordered_inputs(2, 6, 1, 1, 1)))   # 12 x 3
    other = lsq.DeviceMatrix(ctx, rng.standard_normal((m, n + 1)))
    square, qr_sq = solver_on(ctx, rng.standard_normal((n, n)) + 3 * np.eye(n))
    wide, qr_wide = solver_on(ctx, rng.standard_normal((2, n)))
    chol = lsq.AllocatedSolver(dense, lsq.Cholesky(), for_lm=True)
    s2 = C.c_double(0.0)
    o, N = out.ptr, None
    # (label, solver, handle, d_A, p, lda, d_f, d_q, d_se, d_student, d_cook, h_s2, fragment)
    cases = [
        ("every output NULL", qr, dense, N, 0, 0, f.ptr, N, N, N, N, N, "all NULL"),
        ("a Cholesky solver", chol, dense, N, 0, 0, N, o, N, N, N, N, "needs a QR() solver"),
        ("an LSMR solver", lsq.AllocatedSolver(dense, lsq.LSMR(), for_lm=True), dense, N, 0, 0, N, o, N, N, N, N, "needs a QR() solver"),
        ("a CSC handle", qr, csc, N, 0, 0, N, o, N, N, N, N, "not a dense handle"),
        ("a block-diagonal handle", qr, bd, N, 0, 0, N, o, N, N, N, N, "lsq_solver_leverage"),
        ("a bordered handle", qr, bb, N, 0, 0, N, o, N, N, N, N, "not a dense handle"),
        ("another shape", qr, other, N, 0, 0, N, o, N, N, N, N, "allocated for a 12 x 3"),
        ("m < n", qr_wide, wide, N, 0, 0, N, o, N, N, N, N, "needs m >= n"),
        ("m = n with f", qr_sq, square, N, 0, 0, f.ptr, o, N, N, N, N, "needs m > n"),
        ("se without f", qr, dense, N, 0, 0, N, o, o, N, N, N, "need the residual d_f"),
        ("student without f", qr, dense, N, 0, 0, N, N, N, o, N, N, "need the residual d_f"),
        ("cook without f", qr, dense, N, 0, 0, N, N, N, N, o, N, "need the residual d_f"),
        ("s2 without f", qr, dense, N, 0, 0, N, o, N, N, N, C.byref(s2), "need the residual d_f"),
        ("student with new rows", qr, dense, rows.ptr, 2, 2, f.ptr, o, N, o, N, N, "must be NULL"),
        ("cook with new rows", qr, dense, rows.ptr, 2, 2, f.ptr, o, N, N, o, N, "must be NULL"),
        ("p < 1", qr, dense, rows.ptr, 0, 4, N, o, N, N, N, N, "p >= 1 and lda >= p"),
        ("lda < p", qr, dense, rows.ptr, 4, 3, N, o, N, N, N, N, "p >= 1 and lda >= p"),
    ]
    for label, sv, J, pA, p, lda, pf, pq, pse, pt, pck, ps2, fragment in cases:
        rc = L.lsq_dense_qr_leverage(sv.h, J.h, pA, p, lda, pf, pq, pse, pt, pck, ps2, None)
        msg = L.lsq_last_error().decode()
        print(label, "->", rc, msg)
        assert rc == EARG, (label, rc)
        assert msg.startswith("lsq_dense_qr_leverage:") and fragment in msg, (label, msg)
    with pytest.raises(lsq.ArgumentError) as ea:
        chol.dense_qr_leverage()
    assert "needs a QR() solver" in str(ea.value)
    for refused in (bd, bb, csc):                                          # (no QR() solver exists on these handles)
        with pytest.raises(lsq.ArgumentError):
            lsq.dense_qr_leverage(refused)
    # the solver still works after the refusals; m = n without f is served (every leverage is 1)
    r = lc.Ref(np.asfortranarray(A), np.zeros(m))
    ac.judge("dense qr leverage after refusals", lc.pieces("unscaled", qr.dense_qr_leverage().q, r))
    hsq = qr_sq.dense_qr_leverage().q
    assert np.all(np.abs(hsq - 1.0) <= 1e-12)


# ------------------------------------------------------------------------------------------ 9. after a fit: the confidence band
def test_band_after_a_dense_fit(ctx):
    """a exp(-k t) + c with 1 % noise, Dogleg(QR()); then se of the fitted curve at abscissae that were not measured against the
    longdouble reference, and against sqrt(a' Cov a) on the host from lsq_dense_qr_covariance's matrix."""
    m, n = 40, 3
    t = np.linspace(0.0, 4.0, m)
    rng = np.random.default_rng(42)
    data = 1.5 * np.exp(-0.8 * t) + 0.3 + 0.01 * rng.standard_normal(m)

    def f_(out, x):
        out[:] = x[0] * np.exp(-x[1] * t) + x[2] - data

    def rows(x, tt):
        e = np.exp(-x[1] * tt)
        return np.asfortranarray(np.column_stack([e, -x[0] * tt * e, np.ones_like(tt)]))

    def g_(J, x):
        J[:, :] = rows(x, t)

    nls = lsq.LeastSquaresProblem(x=np.array([1.0, 1.0, 0.0]), y=np.zeros(m), f_=f_, g_=g_, J=np.zeros((m, n), order="F"))
    res = lsq.optimize_(nls, lsq.Dogleg(lsq.QR()), ctx=ctx)
    assert res.converged
    x = np.array(res.minimizer)
    Jf, fcur = rows(x, t), np.zeros(m)
    f_(fcur, x)
    Anew = rows(x, np.linspace(-0.5, 6.0, 23))
    Jd = lsq.DeviceMatrix(ctx, Jf)
    band = lsq.dense_qr_leverage(Jd, f=fcur, A=Anew)
    r = lc.Ref(Jf, fcur, A=Anew)
    ac.judge("dense qr leverage band after a fit", lc.pieces("band", band.q, r, True, band.se))
    cov = lsq.dense_qr_covariance(Jd, f=fcur)
    Al, Cl = hp.ld(Anew), hp.ld(cov.cov)
    var_host = np.einsum("ij,jk,ik->i", Al, Cl, Al)
    se_host = np.sqrt(var_host)
    # Cov is within the rule entry by entry, relative to sqrt(C_ii C_jj) >= |C_ij|; the quadratic form a' Cov a adds terms of
    # both signs, so its relative error is that times amp = max_a sum |a_i| sqrt(C_ii C_jj) |a_j| / (a' Cov a) -- the floor of
    # the rule is scaled by it, as ac.trajectory_bound does for a quantity whose condition number is not 1
    sd = np.sqrt(np.diag(Cl))
    amp = float(np.max((np.abs(Al) @ sd) ** 2 / var_host))
    e_ref = lc.lev_err(np.sqrt(r.s2 * r.q_ref), np.sqrt(r.s2_hp * r.q_hp))
    e = lc.lev_err(band.se, se_host)
    print("band against sqrt(a' Cov a): e %.3e, amplification %.1f, bound %.3e" % (e, amp, ac.trajectory_bound(e_ref, n, 1, cond=amp)))
    assert e <= ac.trajectory_bound(e_ref, n, 1, cond=amp)
    own = lsq.dense_qr_leverage(Jd, f=fcur)
    print("fit x %s | se of the curve %.3e .. %.3e | max leverage %.3f max |t| %.2f max cook %.3f"
          % (x, band.se.min(), band.se.max(), own.h.max(), np.abs(own.studentized).max(), own.cook.max()))
    assert abs(own.h.sum() - n) <= 1e-12 and np.all(band.se < 0.1) and np.all(np.abs(own.studentized) < 4)


# ------------------------------------------------------------------------------------------ 10. block-diagonal handle
def bd_solver(ctx, J):
    Jd = lsq.DeviceMatrix(ctx, J)
    return Jd, lsq.AllocatedSolver(Jd, lsq.Cholesky(), for_lm=True)


def check_blocks(label, lev, op, f, scaled=False):
    """h, se and s_b^2 per block by the rule (every block up to B = 7; of more, the first two, the middle one and the last:
    the longdouble reference is the slow part); student and cook against the twin of k_lev_diag on the device's own h and
    s2, on every row."""
    J = op.J
    B, mb, nb = J.nblocks, J.mb, J.nb
    assert np.array_equal(lev.info, np.zeros(B, dtype=np.int32))
    out = []
    for b in (range(B) if B <= 7 else (0, 1, B // 2, B - 1)):
        sl = slice(b * mb, (b + 1) * mb)
        eff = ac.bd_effective(op, b, True) if scaled else None
        r = lc.Ref(np.asfortranarray(J.block(b)), f[sl], J_eff=eff)
        blk = lev.block(b)
        out += lc.pieces("block %d" % b, blk.q, r, True, blk.se)
        out.append(("block %d s2" % b, abs(hp.LD(blk.s2) - r.s2_hp) / r.s2_hp, abs(hp.LD(r.s2) - r.s2_hp) / r.s2_hp, nb))
    se, t, cook = lc.diag_twin(lev.q, f, np.repeat(lev.s2, mb), nb)
    assert np.array_equal(lev.se, se) and np.array_equal(lev.studentized, t) and np.array_equal(lev.cook, cook)
    ac.judge(label, out)


@pytest.mark.parametrize("family", ac.FAMILIES)
@pytest.mark.parametrize("nb", ac.BD_NBS)
def test_blockdiag_accuracy(ctx, nb, family):
    """`ill` (cond(J_b) = 1e3) is the family that tells a CholeskyQR2 from one Cholesky of J_b'J_b: the latter is 15 to 215 x
    beyond the bound at every nb (tests/test_leverage_host.py::test_block_rule_is_within_reach asserts it for the twin)."""
    B, mb = ac.BD_B, ac.BD_MB
    op = ac.bd_operand(family, B, mb, nb, ac.bd_seed(nb))
    f = op.y
    Jd, sv = bd_solver(ctx, op.J)
    lev = sv.leverage(f=f)
    assert np.array_equal(sv.leverage().q, lev.q)
    check_blocks("blockdiag leverage %s nb=%d" % (family, nb), lev, op, f)
    if op.V is not None:                               # graded: also as a column-scaled handle, V diag(s) unrounded
        Jv = lsq.DeviceMatrix(ctx, op.V)
        ds = lsq.DeviceVector(ctx, B * nb, op.s)
        Jv.set_colscale(ds)
        sc = lsq.AllocatedSolver(Jv, lsq.Cholesky(), for_lm=True)
        check_blocks("blockdiag leverage %s nb=%d scaled handle" % (family, nb), sc.leverage(f=f), op, f, scaled=True)


@pytest.mark.parametrize("B", [1, 5, 300])
@pytest.mark.parametrize("mb", [29, 30, 31, 32, 33, 34, 35, 300])
def test_blockdiag_chunk_edges(ctx, B, mb):
    """One to three rows either side of a 32-row chunk, and 300 rows: more than the 256 (64) lanes of the second pass."""
    for nb in (5, 20):
        op = ac.bd_operand("plain", B, mb, nb, 1000 * mb + nb)
        Jd, sv = bd_solver(ctx, op.J)
        check_blocks("blockdiag leverage B=%d mb=%d nb=%d" % (B, mb, nb), sv.leverage(f=op.y), op, op.y)


@pytest.mark.parametrize("nb", [8, 40])
def test_blockdiag_independence_and_repeatability(ctx, nb):
    B, mb = 300, 70
    op = ac.bd_operand("plain", B, mb, nb, 31)
    J, f = op.J, op.y
    Jd, sv = bd_solver(ctx, J)
    keys = ("q", "se", "studentized", "cook", "s2")
    runs = [sv.leverage(f=f) for _ in range(2)]
    lsq.debug_set(serial=1)
    try:
        runs.append(sv.leverage(f=f))
    finally:
        lsq.debug_set(serial=0)
    for other in runs[1:]:
        assert all(np.array_equal(getattr(runs[0], k), getattr(other, k)) for k in keys)
    for b in (0, 2, B - 1):
        one = lsq.BlockDiagonal(1, mb, nb, data=np.asfortranarray(J.block(b)).reshape(-1, order="F"))
        alone = lsq.leverage(lsq.DeviceMatrix(ctx, one), f=f[b * mb:(b + 1) * mb])
        blk = runs[0].block(b)
        for k in ("q", "se", "studentized", "cook"):
            assert np.array_equal(getattr(alone, k), getattr(blk, k)), (b, k)
        assert alone.s2[0] == blk.s2
    # the derived outputs without d_h and d_s2 (the solver's own buffer): the same bits
    dse = lsq.DeviceVector(ctx, B * mb)
    lsq._lib.check(lsq.lib().lsq_solver_leverage(sv.h, Jd.h, lsq.DeviceVector(ctx, B * mb, f).ptr, None, dse.ptr, None, None, None, None))
    assert np.array_equal(dse.get(), runs[0].se)


@pytest.mark.parametrize("nb,k", [(5, 2), (20, 17)])
def test_blockdiag_failing_block(ctx, nb, k):
    """An all-zero column has an exactly zero Gram pivot: block 3 reports column k + 1 and is NaN in every output, the call
    succeeds, and the other blocks carry the bits of the same call on the handle without the defect."""
    B, mb = 6, 70
    good = ac.bd_operand("plain", B, mb, nb, 21).J
    bad = ac.bd_operand("plain", B, mb, nb, 21).J
    bad.block(3)[:, k] = 0.0
    f = np.random.default_rng(nb).standard_normal(B * mb)
    lg = lsq.leverage(lsq.DeviceMatrix(ctx, good), f=f)
    lb = lsq.leverage(lsq.DeviceMatrix(ctx, bad), f=f)
    assert list(lb.info) == [0, 0, 0, k + 1, 0, 0] and np.isnan(lb.s2[3])
    for key in ("q", "se", "studentized", "cook"):
        assert np.all(np.isnan(getattr(lb.block(3), key))), key
        for b in (0, 1, 2, 4, 5):
            assert np.array_equal(getattr(lb.block(b), key), getattr(lg.block(b), key)), (key, b)
    assert np.array_equal(np.delete(lb.s2, 3), np.delete(lg.s2, 3))
    hb = lsq.leverage(lsq.DeviceMatrix(ctx, bad))
    assert list(hb.info) == [0, 0, 0, k + 1, 0, 0] and np.all(np.isnan(hb.block(3).q))


def test_blockdiag_refusals(ctx):
    L = lsq.lib()
    B, mb, nb = 4, 10, 3
    make = lambda B_, mb_, nb_: lsq.BlockDiagonal(B_, mb_, nb_, data=lsq.synthetic.blockdiag_inputs(B_, mb_, nb_, 1))
    Jd = lsq.DeviceMatrix(ctx, make(B, mb, nb))
    out = lsq.DeviceVector(ctx, B * 64)
    f = lsq.DeviceVector(ctx, B * 64)
    chol = lsq.AllocatedSolver(Jd, lsq.Cholesky(), for_lm=True)
    dense = lsq.DeviceMatrix(ctx, np.eye(6, 3))
    import scipy.sparse as sp
    csc = lsq.DeviceMatrix(ctx, sp.csc_matrix(np.eye(6, 3)))
    op = lsq.DeviceOperator(ctx, 6, 3, lambda trans, x, out_: 0, lambda out_: 0)
    other = lsq.DeviceMatrix(ctx, make(B, mb, 2))
    square = lsq.DeviceMatrix(ctx, make(B, nb, nb))
    bb = lsq.DeviceMatrix(ctx, lsq.BorderedBlockDiagonal(B, mb, nb, 2, data=lsq.synthetic.bordered_inputs(B, mb, nb, 2, 1)))
    o, N = out.ptr, None
    # (label, solver, handle, d_f, d_h, d_se, d_student, d_cook, d_s2, fragment)
    cases = [
        ("a bordered handle", chol, bb, N, o, N, N, N, N, "lsq_bordered_qr_covariance"),
        ("a dense handle", lsq.AllocatedSolver(dense, lsq.QR(), for_lm=False), dense, N, o, N, N, N, N, "lsq_dense_qr_leverage"),
        ("a CSC handle", lsq.AllocatedSolver(csc, lsq.LSMR(), for_lm=True), csc, N, o, N, N, N, N, "lsq_sparse_covariance"),
        ("an operator handle", chol, op, N, o, N, N, N, N, "operator handle"),
        ("an LSMR solver", lsq.AllocatedSolver(Jd, lsq.LSMR(), for_lm=True), Jd, N, o, N, N, N, N, "needs a Cholesky() solver"),
        ("a BlockQR solver", lsq.AllocatedSolver(Jd, lsq.BlockQR(), for_lm=True), Jd, N, o, N, N, N, N, "needs a Cholesky() solver"),
        ("another shape", chol, other, N, o, N, N, N, N, "allocated for a block-diagonal Jacobian of 4 blocks of 10 x 3"),
        ("every output NULL", chol, Jd, f.ptr, N, N, N, N, N, "all NULL"),
        ("mb <= nb with f", lsq.AllocatedSolver(square, lsq.Cholesky(), for_lm=True), square, f.ptr, o, N, N, N, N, "needs mb > nb"),
        ("se without f", chol, Jd, N, o, o, N, N, N, "need the residual d_f"),
        ("student without f", chol, Jd, N, N, N, o, N, N, "need the residual d_f"),
        ("cook without f", chol, Jd, N, N, N, N, o, N, "need the residual d_f"),
        ("s2 without f", chol, Jd, N, o, N, N, N, o, "need the residual d_f"),
    ]
    for label, sv, J, pf, ph, pse, pt, pck, ps2, fragment in cases:
        rc = L.lsq_solver_leverage(sv.h, J.h, pf, ph, pse, pt, pck, ps2, None)
        msg = L.lsq_last_error().decode()
        print(label, "->", rc, msg)
        assert rc == EARG, (label, rc)
        assert msg.startswith("lsq_solver_leverage:") and fragment in msg, (label, msg)
    with pytest.raises(lsq.ArgumentError):                                 # ... and as the Python exception
        lsq.leverage(dense)
    # the solver still works after the refusals; mb = nb without f is served (every leverage is 1)
    assert np.array_equal(chol.leverage().info, np.zeros(B, dtype=np.int32))
    hsq = lsq.leverage(square).q
    assert np.all(np.abs(hsq - 1.0) <= 1e-9)


def test_leverages_after_a_batched_fit(ctx):
    """B exponential decays fitted at once (optimize_batched_), then leverages, studentized residuals and Cook's distances at
    the solution, per block, against the longdouble reference on the final Jacobian."""
    B, mb, nb = 5, 30, 2
    t = np.linspace(0.0, 4.0, mb)
    rng = np.random.default_rng(42)
    a, k = 1.0 + rng.random(B), 0.5 + rng.random(B)
    data = a[:, None] * np.exp(-k[:, None] * t) + 0.01 * rng.standard_normal((B, mb))

    def model(x):
        return x[0::2, None] * np.exp(-x[1::2, None] * t)

    def f_(out, x):
        out[:] = (model(x) - data).reshape(-1)

    def jac(x):
        e = np.exp(-x[1::2, None] * t)
        return np.stack([e, -x[0::2, None] * t * e], axis=1)               # [block][column][row]

    def g_(J, x):
        J.data[:] = jac(x).reshape(-1)

    nls = lsq.LeastSquaresProblem(x=np.tile([1.0, 1.0], B), y=np.zeros(B * mb), f_=f_, g_=g_, J=lsq.BlockDiagonal(B, mb, nb))
    res = lsq.optimize_batched_(nls, lsq.LevenbergMarquardt(lsq.Cholesky()), iterations=100, ctx=ctx)
    assert all(res.block(b).converged for b in range(B))
    x = res.minimizer
    Jf = lsq.BlockDiagonal(B, mb, nb, data=jac(x).reshape(-1))
    fres = (model(x) - data).reshape(-1)
    lev = lsq.leverage(lsq.DeviceMatrix(ctx, Jf), f=fres)
    check_blocks("blockdiag leverage after a batched fit", lev, ac.Operand(Jf, fres, None), fres)
    for b in range(B):
        blk = lev.block(b)
        assert abs(blk.h.sum() - nb) <= 1e-12 and np.all(blk.h > 0) and np.all(blk.h < 1)
        assert np.all(np.abs(blk.studentized) < 5) and np.all(blk.cook >= 0)
