"""BorderedQR() on bordered block-diagonal Jacobians on the device (lsq_borderedqr.hip: k_bdq_factor, k_bdq_apply, the inner
dense QR() solver, k_bdq_back), case for case what tests/test_r_gpu_schur.py asks of Schur(): every kernel branch against the
fp64 Householder solve of the stacked matrix, the accuracy tier's rule -- on the five families and on the six-decade `ill6`
family, where Schur() on the same operand is outside the bound --, agreement with Schur() on well-conditioned operands,
LSQ_ERANK with the stacked column, bits, the column-scaled handle, the give-up of the inner QR()'s exchanges, the LM loop
against Schur() and on a graded fit, and every refusal.

Tolerances are the project's: one direct solve rel 1e-9 (tests/gpu_common.py, as tests/test_r_gpu_schur.py uses it), the
accuracy tier's rule accuracy_common.judge (factor 16) with x_hp = the longdouble Householder solve of the stacked matrix and
e_ref = the fp64 Householder solve of the same (tests/borderedqr_common.py), loop iterates to 1e-8.  The cases and the numpy
twin that certifies them on the CPU are in tests/borderedqr_common.py / tests/test_borderedqr_host.py."""
import ctypes as C

import numpy as np
import pytest

import accuracy_common as ac
import borderedqr_common as bq
import schur_common as sc
from gpu_common import lsq

pytestmark = pytest.mark.gpu

PATH = "bordered-qr"


def dev_solve(ctx, Jd, y, damp, sv=None, solver=None):
    sv = sv or lsq.AllocatedSolver(Jd, solver or lsq.BorderedQR(), for_lm=True)
    dx = lsq.DeviceVector(ctx, Jd.n)
    dd = lsq.DeviceVector(ctx, Jd.n, damp)
    _, nmul = sv.ldiv_(dx, lsq.DeviceVector(ctx, Jd.m, y), dd)
    return dx.get(), nmul, sv, dd


# ------------------------------------------------------------------------------------------ 1. every branch
@pytest.mark.parametrize("B,mb,nb,ng", sc.SOLVE_SHAPES)
def test_damped_solve_every_branch(ctx, B, mb, nb, ng):
    J, y, damp = sc.solve_operand(B, mb, nb, ng)
    Jd = lsq.DeviceMatrix(ctx, J)
    x, nmul, sv, dd = dev_solve(ctx, Jd, y, damp)
    err = sc.rel_err(x, bq.qr_fp64_solve_any(J, y, damp))
    info = sv.info()
    print("bordered-qr B=%d mb=%d nb=%d ng=%d rel err %.3e inner %s / %s" % (B, mb, nb, ng, err, info["qr_path"], info["qr_panel"]))
    assert err <= sc.SOLVE_RTOL
    assert nmul == 1
    assert np.array_equal(dd.get(), damp)                  # not written
    assert info["blockdiag_path"] == PATH and info["blockdiag_block"] == -1
    assert info["qr_rank"] == B * nb + ng                  # the locals have full rank, the damped shared part too
    M = B * mb + ng                                        # the inner QR()'s stacked rows: qr2_applies (lsq_qr_stage1.hip)
    two_stage = ng >= 2 and ((ng >= 16 and M * ng >= 1600) or M * ng >= 20000)
    assert info["qr_path"] in (("two-stage-pivoted", "two-stage-certified") if two_stage else ("one-stage",))


# ------------------------------------------------------------------------------------------ 2. the accuracy tier's rule
@pytest.mark.parametrize("family,shape", sc.acc_cases())
def test_accuracy_rule(ctx, family, shape):
    B, mb, nb, ng = shape
    for zero in ((False, True) if family == "ill" else (False,)):
        op, damp, ref = bq.acc_reference(family, shape, zero)
        x, _, sv, _ = dev_solve(ctx, lsq.DeviceMatrix(ctx, op.J), op.y, damp)
        assert sv.info()["blockdiag_path"] == PATH and sv.info()["blockdiag_block"] == -1
        ac.judge("bordered-qr %s B=%d nb=%d ng=%d%s" % (family, B, nb, ng, " zero damping" if zero else ""), ref.pieces(x))
    if family == "graded":
        op, damp, ref = bq.acc_reference(family, shape, False, True)
        Jd = lsq.DeviceMatrix(ctx, op.V)
        Jd.set_colscale(lsq.DeviceVector(ctx, Jd.n, op.s))
        x, _, _, _ = dev_solve(ctx, Jd, op.y, damp)
        ac.judge("bordered-qr %s B=%d nb=%d ng=%d colscale" % (family, B, nb, ng), ref.pieces(x))


@pytest.mark.parametrize("shape", bq.ILL6_SHAPES)
def test_accuracy_rule_six_decades_and_schur_is_outside_it(ctx, shape):
    """cond(J'J) = 1e12: BorderedQR() is inside the bound of the fp64 Householder solve under both right-hand sides, Schur()
    on the same handle is not (it returns, or it stops with a PosDefException: either way it is no answer within the bound)."""
    B, mb, nb, ng = shape
    ops, ref = bq.ill6_reference(shape)
    Jd = lsq.DeviceMatrix(ctx, ops[ac.RHS[0]].J)
    for col, rhs in enumerate(ac.RHS):
        op = ops[rhs]
        x, _, sv, _ = dev_solve(ctx, Jd, op.y, op.damp)
        assert sv.info()["blockdiag_path"] == PATH
        ac.judge("bordered-qr ill6 B=%d nb=%d ng=%d %s" % (B, nb, ng, rhs), ref.pieces(x, col))
        try:
            xs = dev_solve(ctx, Jd, op.y, op.damp, solver=lsq.Schur())[0]
            over = bq.beyond(ref.pieces(xs, col))
        except lsq.PosDefException:
            over = np.inf
        print("   Schur() on the same handle: %.1f x the bound" % over)
        assert over > 1.0, (shape, rhs, over)


# ------------------------------------------------------------------------------------------ 3. agreement with Schur()
@pytest.mark.parametrize("shape", sc.ACC_SHAPES)
def test_agrees_with_schur_on_the_plain_family(ctx, shape):
    """Not bit for bit (another algorithm): within the sum of the two solvers' bounds, piece by piece, in the tier's metric.
    Schur()'s bound is the one its own test holds it to (accuracy_common.bb_solve_pieces: e_ref from the fp64 normal equations)."""
    B, mb, nb, ng = shape
    op, damp, ref = bq.acc_reference("plain", shape)
    Jd = lsq.DeviceMatrix(ctx, op.J)
    xq = dev_solve(ctx, Jd, op.y, damp)[0]
    xs = dev_solve(ctx, Jd, op.y, damp, solver=lsq.Schur())[0]
    pq, ps = ref.pieces(xq), ac.bb_solve_pieces(op, xs, damp)
    ac.judge("BorderedQR() plain B=%d nb=%d ng=%d" % (B, nb, ng), pq)
    ac.judge("Schur() plain B=%d nb=%d ng=%d" % (B, nb, ng), ps)
    for (name, _, rq, k), (_, _, rs, _), d in zip(pq, ps, ref.distance(xq, xs)):
        both = ac.bound(rq, k) + ac.bound(rs, k)
        print("   %s: BorderedQR() vs Schur() %.3e (sum of the two bounds %.3e)" % (name, d, both))
        assert d <= both, (name, d, both)


# ------------------------------------------------------------------------------------------ 4. LSQ_ERANK
@pytest.mark.parametrize("name", bq.RANK_CASES)
def test_rank_failure_reports_the_stacked_column(ctx, name):
    J, y, damp, expect = bq.rank_case(name)
    B, nb = J.nblocks, J.nb
    n, m = J.shape[1], J.shape[0]
    assert expect > 0
    Jd = lsq.DeviceMatrix(ctx, J)
    sv = lsq.AllocatedSolver(Jd, lsq.BorderedQR(), for_lm=True)
    with pytest.raises(lsq.RankDeficientException) as e:
        sv.ldiv_(lsq.DeviceVector(ctx, n), lsq.DeviceVector(ctx, m, y), lsq.DeviceVector(ctx, n, damp))
    assert e.value.status == lsq._lib.ERANK
    assert str(e.value) == bq.ERANK_TEXT % expect, (name, str(e.value))
    info = sv.info()
    assert info["blockdiag_path"] == PATH and info["blockdiag_block"] == (expect - 1) // nb, (name, info)
    # a following clean solve on the same solver and handle is correct
    K, yk, dk, _ = bq.rank_case("good")
    Jd.set_values(K.data)
    x, _, _, _ = dev_solve(ctx, Jd, yk, dk, sv)
    assert sc.rel_err(x, bq.qr_fp64_reference(K, yk, dk)) <= sc.SOLVE_RTOL
    assert sv.info()["blockdiag_block"] == -1


def test_zero_column_with_positive_damping_is_a_solve(ctx):
    J, y, damp, expect = bq.rank_case("damped")
    assert expect == 0
    x, _, sv, _ = dev_solve(ctx, lsq.DeviceMatrix(ctx, J), y, damp)
    assert sc.rel_err(x, bq.qr_fp64_reference(J, y, damp)) <= sc.SOLVE_RTOL
    assert x[2 * J.nb + 1] == 0.0 and sv.info()["blockdiag_block"] == -1      # nothing pulls that parameter away from zero


# ------------------------------------------------------------------------------------------ 5. bits
@pytest.mark.parametrize("B,mb,nb,ng", [(65, 37, 5, 129), (7, 70, 33, 70)])
def test_repeatability_serial_mode_and_jitter(ctx, B, mb, nb, ng):
    J, y, damp = sc.solve_operand(B, mb, nb, ng)
    Jd = lsq.DeviceMatrix(ctx, J)
    x0, _, sv, _ = dev_solve(ctx, Jd, y, damp)
    assert sc.rel_err(x0, bq.qr_fp64_solve_any(J, y, damp)) <= sc.SOLVE_RTOL
    assert np.array_equal(dev_solve(ctx, Jd, y, damp, sv)[0], x0)          # the same solver again
    assert np.array_equal(dev_solve(ctx, Jd, y, damp)[0], x0)              # a second solver on the handle
    lsq.debug_set(serial=1)
    try:
        xs = dev_solve(ctx, Jd, y, damp)[0]
    finally:
        lsq.debug_set(serial=0)
    lsq.debug_set(launch_jitter_us=200)
    try:
        xj = dev_solve(ctx, Jd, y, damp)[0]
    finally:
        lsq.debug_set(launch_jitter_us=0)
    assert np.array_equal(xs, x0) and np.array_equal(xj, x0)


# ------------------------------------------------------------------------------------------ 6. column-scaled handle
@pytest.mark.parametrize("B,mb,nb,ng", [(9, 40, 5, 70), (6, 50, 33, 129), (300, 64, 5, 70), (300, 64, 17, 40)])
def test_column_scaled_handle(ctx, B, mb, nb, ng):
    """J = V diag(s) (lsq_mat_set_colscale) against the unscaled handle that holds fl(V diag(s)).  The first two shapes are
    multiplied out by the handle and small enough for the longdouble reference: both handles are judged by the accuracy rule.
    The last two (nnz >= 2^20: sliced layouts) never are multiplied out -- the kernels apply s to J_b and to the border tiles
    themselves (one wavefront per block / one workgroup per block) -- and are held to the direct-solve tolerance."""
    V, y, damp = sc.solve_operand(B, mb, nb, ng)
    n = B * nb + ng
    rng = np.random.default_rng(B + nb)
    Jd = lsq.DeviceMatrix(ctx, V)
    s = 0.25 + rng.random(n)
    ds = lsq.DeviceVector(ctx, n, s)
    Jd.set_colscale(ds)
    sv = None
    for round_ in range(2):
        J = lsq.BorderedBlockDiagonal(B, mb, nb, ng, data=ac.bb_scale_values(V, s))
        x, _, sv, _ = dev_solve(ctx, Jd, y, damp, sv)
        xu = dev_solve(ctx, lsq.DeviceMatrix(ctx, J), y, damp)[0]
        ref64 = bq.qr_fp64_solve_any(J, y, damp)
        print("column-scaled round %d: vs unscaled handle %.3e, vs fp64 %.3e" % (round_, sc.rel_err(x, xu), sc.rel_err(x, ref64)))
        assert sc.rel_err(x, xu) <= sc.SOLVE_RTOL and sc.rel_err(x, ref64) <= sc.SOLVE_RTOL
        if B * nb + ng <= 400 and round_ == 0:
            op = ac.Operand(J, y, damp, V, s)
            ac.judge("bordered-qr colscale B=%d nb=%d ng=%d scaled handle" % (B, nb, ng), bq.QrPieces(op, damp, y, True).pieces(x))
            ac.judge("bordered-qr colscale B=%d nb=%d ng=%d unscaled handle" % (B, nb, ng), bq.QrPieces(op, damp, y).pieces(xu))
        s = 0.25 + rng.random(n)                           # change s in place and say so
        ds.set(s)
        Jd.colscale_changed()
    Jd.set_colscale(None)
    x, _, _, _ = dev_solve(ctx, Jd, y, damp, sv)
    assert sc.rel_err(x, bq.qr_fp64_solve_any(V, y, damp)) <= sc.SOLVE_RTOL


# ------------------------------------------------------------------------------------------ 7. the inner QR() gives up on an exchange
def test_inner_qr_gives_up_and_repeats_without_exchanges(ctx, monkeypatch):
    B, mb, nb, ng = 9, 40, 5, 200                          # the inner problem is 560 x 200: the blocked two-stage QR
    J, y, damp = sc.solve_operand(B, mb, nb, ng)
    Jd = lsq.DeviceMatrix(ctx, J)
    ref = bq.qr_fp64_reference(J, y, damp)
    clean, _, sv, _ = dev_solve(ctx, Jd, y, damp)
    assert sv.info()["qr_path"] in ("two-stage-pivoted", "two-stage-certified")
    before = sv.stats()["qr_exchange"]
    assert before == {"giveups": 0, "paused": 0}
    monkeypatch.setenv("LSQ_TEST_EXCHANGE_TIMEOUT", "1")
    x, _, _, _ = dev_solve(ctx, Jd, y, damp, sv)
    monkeypatch.delenv("LSQ_TEST_EXCHANGE_TIMEOUT")
    st = sv.stats()["qr_exchange"]
    assert st["giveups"] == 1 and st["paused"] > 0, st     # forwarded from the inner solver
    assert sc.rel_err(clean, ref) <= sc.SOLVE_RTOL and sc.rel_err(x, ref) <= sc.SOLVE_RTOL
    x2, _, _, _ = dev_solve(ctx, Jd, y, damp, sv)          # paused: no exchanges, the same answer
    assert sc.rel_err(x2, ref) <= sc.SOLVE_RTOL
    assert sv.stats()["qr_exchange"]["giveups"] == 1


# ------------------------------------------------------------------------------------------ 8. the LM loop
def _same_run(rs, rd, calls=True):
    assert rs.iterations == rd.iterations
    if calls:
        assert (rs.f_calls, rs.g_calls, rs.mul_calls) == (rd.f_calls, rd.g_calls, rd.mul_calls)
    assert (rs.converged, rs.x_converged, rs.f_converged, rs.g_converged) == (rd.converged, rd.x_converged, rd.f_converged, rd.g_converged)
    assert np.array_equal(rs.trace["accept"], rd.trace["accept"])
    scale = max(1.0, np.max(np.abs(rd.trace["x"])))
    assert np.max(np.abs(rs.trace["x"] - rd.trace["x"])) <= 1e-8 * scale
    assert np.max(np.abs(rs.minimizer - rd.minimizer)) <= 1e-8 * max(1.0, np.max(np.abs(rd.minimizer)))


@pytest.mark.parametrize("B,mb,nb,ng", sc.FITS)
@pytest.mark.parametrize("bounded", [False, True])
def test_lm_matches_schur(ctx, B, mb, nb, ng, bounded):
    fit = sc.TanhFit(B, mb, nb, ng)
    kw, x0 = {}, fit.x0
    if bounded:                                            # one local and one shared weight end on a bound
        free = lsq.optimize_(fit.bordered_problem(), lsq.LevenbergMarquardt(lsq.Schur()), iterations=60, ctx=ctx).minimizer
        lower, upper = np.full(fit.n, -np.inf), np.full(fit.n, np.inf)
        upper[B * nb] = free[B * nb] - 0.05
        lower[2 * nb] = free[2 * nb] + 0.05
        x0 = np.clip(fit.x0, lower, upper)
        kw = dict(lower=lower, upper=upper)
    its = 25 if bounded else 60
    rd = lsq.optimize_(fit.bordered_problem(x0=x0), lsq.LevenbergMarquardt(lsq.Schur()), full_trace=True, iterations=its, ctx=ctx, **kw)
    rs = lsq.optimize_(fit.bordered_problem(x0=x0), lsq.LevenbergMarquardt(lsq.BorderedQR()), full_trace=True, iterations=its, ctx=ctx, **kw)
    print("tanh fit nb=%d ng=%d %s: %d iterations, ssr %.6e" % (nb, ng, "bounded" if bounded else "free", rs.iterations, rs.ssr))
    assert rs.optimizer == "LevenbergMarquardt"
    _same_run(rs, rd)
    if bounded:
        assert np.all(rs.trace["x"] >= lower) and np.all(rs.trace["x"] <= upper)
        assert rs.minimizer[B * nb] == rd.minimizer[B * nb] and rs.minimizer[2 * nb] == rd.minimizer[2 * nb]
    else:
        assert rd.converged
        # BorderedQR() without an optimizer means LevenbergMarquardt
        r0 = lsq.optimize_(fit.bordered_problem(), lsq.api.AbstractOptimizer(lsq.BorderedQR()), iterations=its, ctx=ctx)
        assert r0.optimizer == "LevenbergMarquardt" and r0.iterations == rs.iterations and np.array_equal(r0.minimizer, rs.minimizer)


def test_lm_without_g_and_optimize_with_central_differences(ctx):
    B, mb, nb, ng = sc.FITS[0]
    fit = sc.TanhFit(B, mb, nb, ng)
    rg = lsq.optimize_(fit.bordered_problem(), lsq.LevenbergMarquardt(lsq.BorderedQR()), full_trace=True, iterations=60, ctx=ctx)
    rn = lsq.optimize_(fit.bordered_problem(g=False), lsq.LevenbergMarquardt(lsq.BorderedQR()), full_trace=True, iterations=60, ctx=ctx)
    rd = lsq.optimize_(fit.bordered_problem(g=False), lsq.LevenbergMarquardt(lsq.Schur()), full_trace=True, iterations=60, ctx=ctx)
    _same_run(rn, rd)                                      # central differences under both solvers
    assert rn.converged
    assert np.max(np.abs(rn.minimizer - rg.minimizer)) <= 1e-6 * max(1.0, np.max(np.abs(rg.minimizer)))    # ... against the analytic g!

    def f(x):
        out = np.zeros(fit.m)
        fit.f_(out, x)
        return out

    ro = lsq.optimize(f, fit.x0, lsq.LevenbergMarquardt(lsq.BorderedQR()), autodiff="central", J=lsq.BorderedBlockDiagonal(B, mb, nb, ng),
                      iterations=60, ctx=ctx)
    assert ro.converged and ro.iterations == rn.iterations and np.array_equal(ro.minimizer, rn.minimizer)


def test_allocated_problem_solved_twice(ctx):
    B, mb, nb, ng = sc.FITS[0]
    fit = sc.TanhFit(B, mb, nb, ng)
    ref = lsq.optimize_(fit.bordered_problem(), lsq.LevenbergMarquardt(lsq.BorderedQR()), iterations=60, ctx=ctx)
    nls = fit.bordered_problem()
    nlsa = lsq.LeastSquaresProblemAllocated(nls, lsq.LevenbergMarquardt(lsq.BorderedQR()), ctx=ctx)
    assert isinstance(nlsa.solver, lsq.BorderedQR) and isinstance(nlsa.optimizer, lsq.LevenbergMarquardt)
    try:
        for _ in range(2):
            nlsa.x[:] = fit.x0
            r = lsq.optimize_(nlsa, iterations=60)
            assert r.converged and r.iterations == ref.iterations and np.array_equal(r.minimizer, ref.minimizer)
    finally:
        nlsa.free()


def test_lsq_optimize_from_ctypes(ctx):
    B, mb, nb, ng = sc.FITS[0]
    fit = sc.TanhFit(B, mb, nb, ng)
    ref = lsq.optimize_(fit.bordered_problem(), lsq.LevenbergMarquardt(lsq.BorderedQR()), iterations=60, ctx=ctx)
    L = lsq.lib()
    J = lsq.BorderedBlockDiagonal(B, mb, nb, ng)
    Jd = lsq.DeviceMatrix(ctx, J)
    xh, yh = np.zeros(fit.n), np.zeros(fit.m)

    def fcb(d_out, d_x, user):
        L.lsq_d2h(ctx.h, xh.ctypes.data_as(C.c_void_p), d_x, fit.n * 8)
        fit.f_(yh, xh)
        L.lsq_h2d(ctx.h, d_out, yh.ctypes.data_as(C.c_void_p), fit.m * 8)
        return 0

    def gcb(Jh, d_x, user):
        L.lsq_d2h(ctx.h, xh.ctypes.data_as(C.c_void_p), d_x, fit.n * 8)
        fit.fill(J, xh)
        Jd.set_values(J.data)
        return 0

    F, G = lsq._lib.F_CALLBACK(fcb), lsq._lib.G_CALLBACK(gcb)
    dx, dy = lsq.DeviceVector(ctx, fit.n, fit.x0), lsq.DeviceVector(ctx, fit.m)
    st, res, _ = lsq.api._run_native(ctx, lsq._lib.LEVENBERG_MARQUARDT, lsq._lib.BORDERED_QR, Jd, dx, dy, F, G, None, 1e-8, 1e-8, 1e-8,
                                     60, None, None, None, False, fit.n)
    assert st == 0 and bool(res.converged) and res.iterations == ref.iterations
    assert np.array_equal(dx.get(), ref.minimizer)


def test_lm_converges_on_a_graded_fit(ctx):
    """Feature columns graded over four decades (borderedqr_common.GradedTanhFit): the trace shows the fit converging -- every
    accepted step lowers the sum of squares, the run ends converged, and what is left is the noise: the residual of a fit of n
    parameters to m data with noise sigma has E[ssr] = (m - n) sigma^2 < m sigma^2."""
    B, mb, nb, ng = sc.FITS[0]
    fit = bq.GradedTanhFit(B, mb, nb, ng)
    r = lsq.optimize_(fit.bordered_problem(), lsq.LevenbergMarquardt(lsq.BorderedQR()), full_trace=True, iterations=200, ctx=ctx)
    ssr, acc = r.trace["ssr"], r.trace["accept"]
    print("graded tanh fit: %d iterations, ssr %.6e -> %.6e (m sigma^2 = %.3e), accepted %d" %
          (r.iterations, ssr[0], r.ssr, fit.m * fit.sigma ** 2, int(np.sum(acc))))
    assert r.converged
    assert np.all(np.diff(ssr) <= 0.0) and r.ssr < ssr[0]
    assert r.ssr <= fit.m * fit.sigma ** 2


# ------------------------------------------------------------------------------------------ 9. refusals through the C ABI
def test_refusals_through_the_c_abi(ctx):
    L = lsq.lib()
    last = lambda: L.lsq_last_error().decode()
    J, y, damp = sc.solve_operand(4, 16, 8, 70)
    Jd = lsq.DeviceMatrix(ctx, J)
    n, m = Jd.n, Jd.m

    def still_works(sv=None):
        x, _, _, _ = dev_solve(ctx, Jd, y, damp, sv)
        assert sc.rel_err(x, bq.qr_fp64_reference(J, y, damp)) <= sc.SOLVE_RTOL

    # every other kind of handle
    sp = pytest.importorskip("scipy.sparse")
    others = [(lsq.DeviceMatrix(ctx, np.zeros((6, 3))), "a dense handle", "QR()"),
              (lsq.DeviceMatrix(ctx, sp.random(9, 4, 0.5, format="csc", random_state=1)), "a plain CSC handle", "LSMR()"),
              (lsq.DeviceMatrix(ctx, lsq.BlockDiagonal(3, 4, 2)), "a block-diagonal handle", "BlockQR()"),
              (lsq.DeviceOperator(ctx, 6, 3, lambda *a: None, lambda *a: None), "an operator handle", "LSMR()")]
    for Jo, what, alt in others:
        h = C.c_void_p()
        assert L.lsq_solver_create(ctx.h, Jo.h, lsq._lib.BORDERED_QR, 1, C.byref(h)) == lsq._lib.EARG, what
        assert "BorderedQR() needs a bordered block-diagonal Jacobian" in last() and what in last() and alt in last(), last()
    still_works()
    # nb > 64
    J65 = lsq.DeviceMatrix(ctx, sc.make_bb(2, 70, 65, 5, 1))
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.AllocatedSolver(J65, lsq.BorderedQR(), for_lm=True)
    assert e.value.status == lsq._lib.EARG
    assert "nb <= 64" in str(e.value) and "nb = 65, ng = 5" in str(e.value) and "LSMR()" in str(e.value)
    lsq.AllocatedSolver(J65, lsq.LSMR(), for_lm=True)        # ... LSMR() takes it
    still_works()
    # for_lm = 0, and lsq_ldiv on a solver allocated for LM: the bordered handle's Dogleg text
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.AllocatedSolver(Jd, lsq.BorderedQR(), for_lm=False)
    assert e.value.status == lsq._lib.EARG and str(e.value) == lsq.api.BORDERED_DOGLEG_TEXT
    sv = lsq.AllocatedSolver(Jd, lsq.BorderedQR(), for_lm=True)
    assert sv.info()["qr_rank"] == -1 and sv.info()["blockdiag_path"] is None      # before the first solve
    with pytest.raises(lsq.ArgumentError) as e:
        sv.ldiv_(lsq.DeviceVector(ctx, n), lsq.DeviceVector(ctx, m, y))
    assert e.value.status == lsq._lib.EARG and str(e.value) == lsq.api.BORDERED_DOGLEG_TEXT
    still_works(sv)
    # Dogleg in lsq_optimize: the loop's own solver creation takes the same refusal
    F = lsq._lib.F_CALLBACK(lambda d_out, d_x, user: 0)
    G = lsq._lib.G_CALLBACK(lambda Jh, d_x, user: 0)
    st, _, _ = lsq.api._run_native(ctx, lsq._lib.DOGLEG, lsq._lib.BORDERED_QR, Jd, lsq.DeviceVector(ctx, n), lsq.DeviceVector(ctx, m),
                                   F, G, None, 1e-8, 1e-8, 1e-8, 5, None, None, None, False, n)
    assert st == lsq._lib.EARG and last() == lsq.api.BORDERED_DOGLEG_TEXT
    still_works(sv)
    # lsq_optimize_batched, on the bordered handle and on a block-diagonal one
    for Jh, shape in ((Jd.h, (4, 16, 8)), (others[2][0].h, (3, 4, 2))):
        st, _ = lsq.api._run_native_batched(ctx, lsq._lib.LEVENBERG_MARQUARDT, lsq._lib.BORDERED_QR, Jh, shape, lsq.DeviceVector(ctx, n),
                                            lsq.DeviceVector(ctx, m), F, G, None, 1e-8, 1e-8, 1e-8, 5, None, None, None, False,
                                            "LevenbergMarquardt")
        assert st == lsq._lib.EARG
        assert "lsq_optimize_batched: BorderedQR()" in last() and "lsq_optimize with LevenbergMarquardt" in last()
    still_works(sv)
    # all four covariance entries
    with pytest.raises(lsq.ArgumentError) as e:
        sv.covariance()
    assert e.value.status == lsq._lib.EARG
    assert "not available on a BorderedQR() solver" in str(e.value) and "lsq_sparse_covariance" in str(e.value)
    for entry, word in ((sv.dense_covariance, "lsq_dense_covariance"), (sv.dense_qr_covariance, "lsq_dense_qr_covariance"),
                        (sv.sparse_covariance, "lsq_sparse_covariance")):
        with pytest.raises(lsq.ArgumentError) as e:
            entry()
        assert e.value.status == lsq._lib.EARG and word in str(e.value), str(e.value)
    still_works(sv)
    # a handle of another shape than the solver was created for
    for other in (sc.make_bb(4, 16, 8, 71, 1), sc.make_bb(5, 16, 8, 70, 1), sc.make_bb(4, 17, 8, 70, 1)):
        Jo = lsq.DeviceMatrix(ctx, other)
        sv.J = Jo
        with pytest.raises(lsq.ArgumentError) as e:
            sv.ldiv_(lsq.DeviceVector(ctx, Jo.n), lsq.DeviceVector(ctx, Jo.m), lsq.DeviceVector(ctx, Jo.n, np.ones(Jo.n)))
        assert e.value.status == lsq._lib.EARG
        assert "4 blocks of 16 x 8 with 70 shared columns" in str(e.value) and "create a solver on the handle" in str(e.value)
    sv.J = Jd
    still_works(sv)
