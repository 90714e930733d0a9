"""Schur() on bordered block-diagonal Jacobians on the device (lsq_schur.hip: k_sc_eliminate, the two tall products on the
dense path's SYRK kernel, k_sc_reduce, the inner dense Cholesky() solver, k_sc_back): every kernel branch against the fp64
reference and the dense handle, the accuracy tier's rule, agreement with Cholesky() on the same handle, PosDefException
parity with the dense handle on operands whose failing pivot is exact, bits, the column-scaled handle, the give-up of the
one-launch factorisation, the LM loop against the same fit on the dense handle, and every refusal.

Tolerances are the project's: one direct solve rel 1e-9 (tests/gpu_common.py, as tests/test_f_gpu_bordered.py uses it), the
accuracy tier's rule accuracy_common.judge (factor 16 against the longdouble reference), loop iterates to 1e-8.  The cases and
the numpy twin that certifies them on the CPU are in tests/schur_common.py / tests/test_schur_host.py."""
import ctypes as C

import numpy as np
import pytest

import accuracy_common as ac
import schur_common as sc
from gpu_common import lsq

pytestmark = pytest.mark.gpu

PD_TEXT = "PosDefException: matrix is not positive definite; Cholesky failed at %d"


def dev_solve(ctx, Jd, y, damp, sv=None, solver=None):
    sv = sv or lsq.AllocatedSolver(Jd, solver or lsq.Schur(), for_lm=True)
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
    err = sc.rel_err(x, ac.bb_fp64_solve(J, y, damp))
    info = sv.info()
    print("schur B=%d mb=%d nb=%d ng=%d rel err %.3e inner %s" % (B, mb, nb, ng, err, info["chol_path"]))
    assert err <= sc.SOLVE_RTOL
    assert nmul == 1
    assert np.array_equal(dd.get(), damp)                  # not written
    assert info["blockdiag_path"] == "bordered-schur-tiled" and info["blockdiag_block"] == -1
    blocked = ng >= 32 or (ng >= 2 and B * mb * ng >= 20000)       # lsq_cholesky_takes_blocked
    assert info["chol_path"] in (("blocked", "blocked-one-launch") if blocked else ("one-workgroup",))
    if B * mb * (B * nb + ng) <= sc.DENSE_HANDLE_MAX:
        xd = dev_solve(ctx, lsq.DeviceMatrix(ctx, J.toarray()), y, damp, solver=lsq.Cholesky())[0]
        errd = sc.rel_err(x, xd)
        print("   vs Cholesky() on the dense handle %.3e" % errd)
        assert errd <= sc.SOLVE_RTOL


# ------------------------------------------------------------------------------------------ 2. the accuracy tier's rule
@pytest.mark.parametrize("family,shape", sc.acc_cases())
def test_accuracy_rule(ctx, family, shape):
    B, mb, nb, ng = shape
    op = ac.bb_operand(family, B, mb, nb, ng, sc.acc_seed(B, nb, ng))
    damps = [("", op.damp)] + ([(" zero damping", np.zeros(B * nb + ng))] if family == "ill" else [])
    handles = [("", lsq.DeviceMatrix(ctx, op.J), False)]
    if op.V is not None:
        Jd = lsq.DeviceMatrix(ctx, op.V)
        Jd.set_colscale(lsq.DeviceVector(ctx, Jd.n, op.s))
        handles.append((" colscale", Jd, True))
    for label, Jd, scaled in handles:
        for dlabel, damp in damps:
            x, _, sv, _ = dev_solve(ctx, Jd, op.y, damp)
            assert sv.info()["blockdiag_path"] == "bordered-schur-tiled" and sv.info()["blockdiag_block"] == -1
            ac.judge("schur %s B=%d nb=%d ng=%d%s%s" % (family, B, nb, ng, label, dlabel), ac.bb_solve_pieces(op, x, damp, scaled))


# ------------------------------------------------------------------------------------------ 3. agreement with Cholesky()
@pytest.mark.parametrize("family", ac.FAMILIES)
@pytest.mark.parametrize("nb,ng", sc.AGREE_SHAPES)
def test_agrees_with_cholesky_on_the_same_handle(ctx, nb, ng, family):
    """nb + ng <= 64: both solvers take the handle; not bit for bit (the corner is summed in another order), so both are held
    to the same rule."""
    B, mb = 5, 96
    op = ac.bb_operand(family, B, mb, nb, ng, sc.acc_seed(B, nb, ng))
    Jd = lsq.DeviceMatrix(ctx, op.J)
    xs, _, svs, _ = dev_solve(ctx, Jd, op.y, op.damp)
    xc, _, svc, _ = dev_solve(ctx, Jd, op.y, op.damp, solver=lsq.Cholesky())
    assert svs.info()["blockdiag_path"] == "bordered-schur-tiled" and svc.info()["blockdiag_path"] == "bordered-schur"
    ac.judge("Schur() %s nb=%d ng=%d" % (family, nb, ng), ac.bb_solve_pieces(op, xs, op.damp))
    ac.judge("Cholesky() %s nb=%d ng=%d" % (family, nb, ng), ac.bb_solve_pieces(op, xc, op.damp))
    print("   Schur() vs Cholesky() rel %.3e" % sc.rel_err(xs, xc))


# ------------------------------------------------------------------------------------------ 4. not positive definite
@pytest.mark.parametrize("name", sorted(sc.FAILURES))
def test_not_positive_definite_reports_the_stacked_column(ctx, name):
    J, y, damp = sc.failure_case(name)
    B, nb, ng = J.nblocks, J.nb, J.ng
    n, m = J.shape[1], J.shape[0]
    expect = sc.stacked_potrf_column(J, damp)
    assert expect > 0
    Jd = lsq.DeviceMatrix(ctx, J)
    sv = lsq.AllocatedSolver(Jd, lsq.Schur(), for_lm=True)
    with pytest.raises(lsq.PosDefException) as e:
        sv.ldiv_(lsq.DeviceVector(ctx, n), lsq.DeviceVector(ctx, m, y), lsq.DeviceVector(ctx, n, damp))
    assert e.value.status == lsq._lib.ENOTPD
    assert str(e.value) == PD_TEXT % expect, (name, str(e.value))
    info = sv.info()
    assert info["blockdiag_path"] == "bordered-schur-tiled"
    assert info["blockdiag_block"] == (B if expect > B * nb else (expect - 1) // nb), (name, info)
    with pytest.raises(lsq.PosDefException) as ed:                         # the dense handle says the same
        dense_sv = lsq.AllocatedSolver(lsq.DeviceMatrix(ctx, J.toarray()), lsq.Cholesky(), for_lm=True)
        dense_sv.ldiv_(lsq.DeviceVector(ctx, n), lsq.DeviceVector(ctx, m, y), lsq.DeviceVector(ctx, n, damp))
    assert str(ed.value) == str(e.value)
    # a following clean solve on the same solver and handle is correct
    _, _, _, rows, _ = sc.FAILURES[name]
    K, yk, dk = sc.exact_operand(B, nb, ng, rows)
    Jd.set_values(K.data)
    x, _, _, _ = dev_solve(ctx, Jd, yk, dk, sv)
    assert sc.rel_err(x, ac.bb_fp64_solve(K, yk, dk)) <= sc.SOLVE_RTOL
    assert sv.info()["blockdiag_block"] == -1


# ------------------------------------------------------------------------------------------ 5. bits
@pytest.mark.parametrize("B,mb,nb,ng", [(65, 37, 5, 129), (7, 70, 33, 70)])
def test_repeatability_serial_mode_and_jitter(ctx, B, mb, nb, ng):
    J, y, damp = sc.solve_operand(B, mb, nb, ng)
    Jd = lsq.DeviceMatrix(ctx, J)
    x0, _, sv, _ = dev_solve(ctx, Jd, y, damp)
    assert sc.rel_err(x0, ac.bb_fp64_solve(J, y, damp)) <= sc.SOLVE_RTOL
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
    multiplied out by the handle; the last two (nnz >= 2^20: sliced layouts) never are -- the kernels apply s to G_bb, J_b'y_b,
    J_b'C_b and the corner themselves (one wavefront per block / one workgroup per block)."""
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
        print("column-scaled round %d: vs unscaled handle %.3e, vs fp64 %.3e"
              % (round_, sc.rel_err(x, xu), sc.rel_err(x, ac.bb_fp64_solve(J, y, damp))))
        assert sc.rel_err(x, xu) <= sc.SOLVE_RTOL
        assert sc.rel_err(x, ac.bb_fp64_solve(J, y, damp)) <= sc.SOLVE_RTOL
        s = 0.25 + rng.random(n)                           # change s in place and say so
        ds.set(s)
        Jd.colscale_changed()
    Jd.set_colscale(None)
    x, _, _, _ = dev_solve(ctx, Jd, y, damp, sv)
    assert sc.rel_err(x, ac.bb_fp64_solve(V, y, damp)) <= sc.SOLVE_RTOL


# ------------------------------------------------------------------------------------------ 7. the one-launch factorisation gives up
def test_one_launch_gives_up_and_panels_take_over(ctx, monkeypatch):
    B, mb, nb, ng = 9, 40, 5, 200                          # ng = 200: 10 tiles, which the one-launch factorisation accepts
    J, y, damp = sc.solve_operand(B, mb, nb, ng)
    Jd = lsq.DeviceMatrix(ctx, J)
    ref = ac.bb_fp64_solve(J, y, damp)
    clean, _, sv, _ = dev_solve(ctx, Jd, y, damp)
    assert sv.info()["chol_path"] == "blocked-one-launch"
    before = sv.stats()["chol_one_launch"]["giveups"]
    monkeypatch.setenv("LSQ_TEST_EXCHANGE_TIMEOUT", "1")
    x, _, _, _ = dev_solve(ctx, Jd, y, damp, sv)
    monkeypatch.delenv("LSQ_TEST_EXCHANGE_TIMEOUT")
    assert sv.stats()["chol_one_launch"]["giveups"] == before + 1
    assert sv.info()["chol_path"] == "blocked"
    assert sc.rel_err(clean, ref) <= sc.SOLVE_RTOL and sc.rel_err(x, ref) <= sc.SOLVE_RTOL
    x2, _, _, _ = dev_solve(ctx, Jd, y, damp, sv)          # paused: panel launches, the same answer
    assert sc.rel_err(x2, ref) <= sc.SOLVE_RTOL


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
def test_lm_matches_cholesky_on_the_dense_handle(ctx, B, mb, nb, ng, bounded):
    fit = sc.TanhFit(B, mb, nb, ng)
    kw, x0 = {}, fit.x0
    if bounded:                                            # one local and one shared weight end on a bound
        free = lsq.optimize_(fit.dense_problem(), lsq.LevenbergMarquardt(lsq.Cholesky()), iterations=60, ctx=ctx).minimizer
        lower, upper = np.full(fit.n, -np.inf), np.full(fit.n, np.inf)
        upper[B * nb] = free[B * nb] - 0.05
        lower[2 * nb] = free[2 * nb] + 0.05
        x0 = np.clip(fit.x0, lower, upper)
        kw = dict(lower=lower, upper=upper)
    its = 25 if bounded else 60
    rd = lsq.optimize_(fit.dense_problem(x0), lsq.LevenbergMarquardt(lsq.Cholesky()), full_trace=True, iterations=its, ctx=ctx, **kw)
    rs = lsq.optimize_(fit.bordered_problem(x0=x0), lsq.LevenbergMarquardt(lsq.Schur()), full_trace=True, iterations=its, ctx=ctx, **kw)
    print("tanh fit nb=%d ng=%d %s: %d iterations, ssr %.6e" % (nb, ng, "bounded" if bounded else "free", rs.iterations, rs.ssr))
    assert rs.optimizer == "LevenbergMarquardt"
    _same_run(rs, rd)
    if bounded:
        assert np.all(rs.trace["x"] >= lower) and np.all(rs.trace["x"] <= upper)
        assert rs.minimizer[B * nb] == rd.minimizer[B * nb] and rs.minimizer[2 * nb] == rd.minimizer[2 * nb]
    else:
        assert rd.converged
        # Schur() without an optimizer means LevenbergMarquardt
        r0 = lsq.optimize_(fit.bordered_problem(), lsq.api.AbstractOptimizer(lsq.Schur()), iterations=its, ctx=ctx)
        assert r0.optimizer == "LevenbergMarquardt" and r0.iterations == rs.iterations and np.array_equal(r0.minimizer, rs.minimizer)


def test_lm_without_g_and_optimize_with_central_differences(ctx):
    B, mb, nb, ng = sc.FITS[0]
    fit = sc.TanhFit(B, mb, nb, ng)
    rg = lsq.optimize_(fit.bordered_problem(), lsq.LevenbergMarquardt(lsq.Schur()), full_trace=True, iterations=60, ctx=ctx)
    rn = lsq.optimize_(fit.bordered_problem(g=False), lsq.LevenbergMarquardt(lsq.Schur()), full_trace=True, iterations=60, ctx=ctx)
    dense = lsq.LeastSquaresProblem(x=fit.x0.copy(), y=np.zeros(fit.m), f_=fit.f_, J=np.zeros((fit.m, fit.n), order="F"))
    rd = lsq.optimize_(dense, lsq.LevenbergMarquardt(lsq.Cholesky()), full_trace=True, iterations=60, ctx=ctx)
    _same_run(rn, rd, calls=False)                         # central differences on both handles (which count their f! calls apart)
    assert (rn.g_calls, rn.mul_calls) == (rd.g_calls, rd.mul_calls)
    assert rn.converged
    assert np.max(np.abs(rn.minimizer - rg.minimizer)) <= 1e-6 * max(1.0, np.max(np.abs(rg.minimizer)))    # ... against the analytic g!

    def f(x):
        out = np.zeros(fit.m)
        fit.f_(out, x)
        return out

    ro = lsq.optimize(f, fit.x0, lsq.LevenbergMarquardt(lsq.Schur()), autodiff="central", J=lsq.BorderedBlockDiagonal(B, mb, nb, ng),
                      iterations=60, ctx=ctx)
    assert ro.converged and ro.iterations == rn.iterations and np.array_equal(ro.minimizer, rn.minimizer)


def test_allocated_problem_solved_twice(ctx):
    B, mb, nb, ng = sc.FITS[0]
    fit = sc.TanhFit(B, mb, nb, ng)
    ref = lsq.optimize_(fit.bordered_problem(), lsq.LevenbergMarquardt(lsq.Schur()), iterations=60, ctx=ctx)
    nls = fit.bordered_problem()
    nlsa = lsq.LeastSquaresProblemAllocated(nls, lsq.LevenbergMarquardt(lsq.Schur()), ctx=ctx)
    assert isinstance(nlsa.solver, lsq.Schur) and isinstance(nlsa.optimizer, lsq.LevenbergMarquardt)
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
    ref = lsq.optimize_(fit.bordered_problem(), lsq.LevenbergMarquardt(lsq.Schur()), iterations=60, ctx=ctx)
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
    st, res, _ = lsq.api._run_native(ctx, lsq._lib.LEVENBERG_MARQUARDT, lsq._lib.SCHUR, Jd, dx, dy, F, G, None, 1e-8, 1e-8, 1e-8, 60,
                                     None, None, None, False, fit.n)
    assert st == 0 and bool(res.converged) and res.iterations == ref.iterations
    assert np.array_equal(dx.get(), ref.minimizer)


# ------------------------------------------------------------------------------------------ 9. refusals through the C ABI
def test_refusals_through_the_c_abi(ctx):
    L = lsq.lib()
    last = lambda: L.lsq_last_error().decode()
    J, y, damp = sc.solve_operand(4, 16, 8, 70)
    Jd = lsq.DeviceMatrix(ctx, J)
    n, m = Jd.n, Jd.m

    def still_works(sv=None):
        x, _, _, _ = dev_solve(ctx, Jd, y, damp, sv)
        assert sc.rel_err(x, ac.bb_fp64_solve(J, y, damp)) <= sc.SOLVE_RTOL

    # every other kind of handle
    sp = pytest.importorskip("scipy.sparse")
    others = [(lsq.DeviceMatrix(ctx, np.zeros((6, 3))), "a dense handle", "Cholesky() or QR()"),
              (lsq.DeviceMatrix(ctx, sp.random(9, 4, 0.5, format="csc", random_state=1)), "a plain CSC handle", "LSMR()"),
              (lsq.DeviceMatrix(ctx, lsq.BlockDiagonal(3, 4, 2)), "a block-diagonal handle", "Cholesky() or BlockQR()"),
              (lsq.DeviceOperator(ctx, 6, 3, lambda *a: None, lambda *a: None), "an operator handle", "LSMR()")]
    for Jo, what, alt in others:
        h = C.c_void_p()
        assert L.lsq_solver_create(ctx.h, Jo.h, lsq._lib.SCHUR, 1, C.byref(h)) == lsq._lib.EARG, what
        assert "Schur() needs a bordered block-diagonal Jacobian" in last() and what in last() and alt in last(), last()
    still_works()
    # nb > 64
    J65 = lsq.DeviceMatrix(ctx, sc.make_bb(2, 70, 65, 5, 1))
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.AllocatedSolver(J65, lsq.Schur(), for_lm=True)
    assert e.value.status == lsq._lib.EARG
    assert "nb <= 64" in str(e.value) and "nb = 65, ng = 5" in str(e.value) and "LSMR()" in str(e.value)
    lsq.AllocatedSolver(J65, lsq.LSMR(), for_lm=True)        # ... LSMR() takes it
    still_works()
    # for_lm = 0, and lsq_ldiv on a solver allocated for LM: the bordered handle's Dogleg text
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.AllocatedSolver(Jd, lsq.Schur(), for_lm=False)
    assert e.value.status == lsq._lib.EARG and str(e.value) == lsq.api.BORDERED_DOGLEG_TEXT
    sv = lsq.AllocatedSolver(Jd, lsq.Schur(), for_lm=True)
    with pytest.raises(lsq.ArgumentError) as e:
        sv.ldiv_(lsq.DeviceVector(ctx, n), lsq.DeviceVector(ctx, m, y))
    assert e.value.status == lsq._lib.EARG and str(e.value) == lsq.api.BORDERED_DOGLEG_TEXT
    still_works(sv)
    # Dogleg in lsq_optimize: the loop's own solver creation takes the same refusal
    F = lsq._lib.F_CALLBACK(lambda d_out, d_x, user: 0)
    G = lsq._lib.G_CALLBACK(lambda Jh, d_x, user: 0)
    st, _, _ = lsq.api._run_native(ctx, lsq._lib.DOGLEG, lsq._lib.SCHUR, Jd, lsq.DeviceVector(ctx, n), lsq.DeviceVector(ctx, m),
                                   F, G, None, 1e-8, 1e-8, 1e-8, 5, None, None, None, False, n)
    assert st == lsq._lib.EARG and last() == lsq.api.BORDERED_DOGLEG_TEXT
    still_works(sv)
    # lsq_optimize_batched, on the bordered handle and on a block-diagonal one
    for Jh, shape in ((Jd.h, (4, 16, 8)), (others[2][0].h, (3, 4, 2))):
        st, _ = lsq.api._run_native_batched(ctx, lsq._lib.LEVENBERG_MARQUARDT, lsq._lib.SCHUR, Jh, shape, lsq.DeviceVector(ctx, n),
                                            lsq.DeviceVector(ctx, m), F, G, None, 1e-8, 1e-8, 1e-8, 5, None, None, None, False,
                                            "LevenbergMarquardt")
        assert st == lsq._lib.EARG
        assert "lsq_optimize_batched: Schur()" in last() and "lsq_optimize with LevenbergMarquardt" in last()
    still_works(sv)
    # lsq_solver_covariance
    with pytest.raises(lsq.ArgumentError) as e:
        sv.covariance()
    assert e.value.status == lsq._lib.EARG
    assert "not available on a Schur() solver" in str(e.value) and "lsq_sparse_covariance" in str(e.value)
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
