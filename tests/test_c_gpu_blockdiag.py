"""Block-diagonal Jacobians on the device: the handle (lsq_blockdiag_create: a CSC handle that knows its block shape) and
Cholesky() on it (lsq_blockdiag.hip: B independent nb x nb normal-equation solves in one pass over the values) against the
oracle on the STACKED dense matrix, numpy per block, and the dense handle's own Cholesky() on the device.

Tolerances are the project's (tests/gpu_common.py): kernels 1e-12 * scale, one direct solve rel 1e-9, trajectories through
compare_until_roundoff with its defaults.  Operands: the library's N(0,1)/sqrt(mb) generator (cond(J_b'J_b) ~ 10 at 128 x 32).

The pivoted (Dogleg) factorisation follows the reference, which passes tol = 0.0 to dpstrf (oracle/lsq_oracle.c:601-611,
tests/test_b_gpu_kernels.py::test_ldiv_cholesky_dogleg_certificate): it stops when the largest remaining pivot is <= 0, so
a generic duplicated column leaves a pivot of rounding noise whose sign nobody controls.  The rank-deficient operand below
is a duplicated column whose elimination is EXACT in binary floating point (see test_undamped_solve_and_rank_deficiency)."""
import numpy as np
import pytest

from gpu_common import compare_until_roundoff, lsq
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SOLVE_RTOL = 1e-9        # gpu_common: one direct solve
KERNEL_TOL = 1e-12       # gpu_common: kernels, times the scale of the result


def make_bd(B, mb, nb, seed):
    return lsq.BlockDiagonal(B, mb, nb, data=lsq.synthetic.blockdiag_inputs(B, mb, nb, seed))


def blocks_solve(J, y, damp=None):
    """numpy.linalg.solve(J_b'J_b + D_b, J_b'y_b) block by block."""
    x = np.zeros(J.shape[1])
    for b in range(J.nblocks):
        A = J.block(b)
        G = A.T @ A
        if damp is not None:
            G = G + np.diag(damp[b * J.nb:(b + 1) * J.nb])
        x[b * J.nb:(b + 1) * J.nb] = np.linalg.solve(G, A.T @ y[b * J.mb:(b + 1) * J.mb])
    return x


def rel_err(x, ref):
    return np.linalg.norm(x - ref) / np.linalg.norm(ref)


def dev_solve(ctx, Jd, y, damp=None, for_lm=None):
    sv = lsq.AllocatedSolver(Jd, lsq.Cholesky(), for_lm=(damp is not None) if for_lm is None else for_lm)
    dx = lsq.DeviceVector(ctx, Jd.n)
    dd = lsq.DeviceVector(ctx, Jd.n, damp) if damp is not None else None
    _, nmul = sv.ldiv_(dx, lsq.DeviceVector(ctx, Jd.m, y), dd)
    return dx.get(), nmul, sv, dd


# ------------------------------------------------------------------------------------------ 1. the handle is a CSC handle
@pytest.mark.parametrize("B,mb,nb", [(16, 128, 32), (7, 3, 5), (300, 257, 17)])
def test_handle_is_a_csc_handle(ctx, B, mb, nb):
    J = make_bd(B, mb, nb, 3)
    Jd = lsq.DeviceMatrix(ctx, J)
    assert Jd.blockdiag_info() == (B, mb, nb) and (Jd.m, Jd.n, Jd.nnz) == (B * mb, B * nb, B * mb * nb)
    Jo = O.Mat.from_scipy(J.tocsc())
    rng = np.random.default_rng(B)
    x, y = rng.standard_normal(Jd.n), rng.standard_normal(Jd.m)
    y0, x0 = rng.standard_normal(Jd.m), rng.standard_normal(Jd.n)
    dx, dy = lsq.DeviceVector(ctx, Jd.n, x), lsq.DeviceVector(ctx, Jd.m, y)
    for alpha, beta in ((1.0, 0.0), (-0.75, 0.0), (2.5, -0.5)):
        out = lsq.DeviceVector(ctx, Jd.m, y0)
        lsq.mul_(out, Jd, dx, alpha, beta)
        ref = O.mul(Jo, x, alpha, beta, y0)
        assert np.max(np.abs(out.get() - ref)) <= KERNEL_TOL * max(1.0, np.max(np.abs(ref))), (alpha, beta)
        out = lsq.DeviceVector(ctx, Jd.n, x0)
        lsq.mul_(out, Jd, dy, alpha, beta, trans=True)
        ref = O.mulT(Jo, y, alpha, beta, x0)
        assert np.max(np.abs(out.get() - ref)) <= KERNEL_TOL * max(1.0, np.max(np.abs(ref))), (alpha, beta, "T")
    cs = lsq.colsumabs2_(lsq.DeviceVector(ctx, Jd.n), Jd).get()
    ref = O.colsumabs2(Jo)
    assert np.max(np.abs(cs - ref)) <= KERNEL_TOL * np.max(ref)
    rs = lsq.rowsumabs2_(lsq.DeviceVector(ctx, Jd.m), Jd).get()
    ref = O.rowsumabs2(Jo)
    assert np.max(np.abs(rs - ref)) <= KERNEL_TOL * np.max(ref)
    # values round trip, in the container's order
    assert np.array_equal(Jd.values(), J.data)
    v2 = rng.standard_normal(J.nnz)
    Jd.set_values(v2)
    assert np.array_equal(Jd.values(), v2)
    # a handle that is not block-diagonal says so
    assert lsq.DeviceMatrix(ctx, J.tocsc()).blockdiag_info() == (0, 0, 0)
    assert lsq.DeviceMatrix(ctx, np.zeros((4, 3))).blockdiag_info() == (0, 0, 0)


# ------------------------------------------------------------------------------------------ 2. one damped solve
@pytest.mark.parametrize("nb", [1, 5, 16, 17, 32, 48, 64])
def test_damped_solve_every_shape(ctx, nb):
    """lsq_ldiv_damped, every kernel branch: one wavefront per block (nb <= 16) and one workgroup per block with 2, 3, 4 tile
    rows; mb below one chunk, two chunks, a ragged ninth chunk (mb < nb included: the damping makes it solvable); a single
    block, a grid that ends inside a workgroup of four (7) and 300 blocks."""
    for mb in (3, 64, 257):
        for B in (1, 7, 300):
            J = make_bd(B, mb, nb, 1000 * nb + mb + B)
            rng = np.random.default_rng(nb * mb + B)
            y = rng.standard_normal(B * mb)
            damp = 0.05 + rng.random(B * nb)
            x, nmul, sv, dd = dev_solve(ctx, lsq.DeviceMatrix(ctx, J), y, damp)
            ref = blocks_solve(J, y, damp)
            err = rel_err(x, ref)
            print("damped nb=%d mb=%d B=%d rel err %.3e" % (nb, mb, B, err))
            assert err <= SOLVE_RTOL, (nb, mb, B, err)
            assert nmul == 1
            assert np.array_equal(dd.get(), damp)          # not clobbered (dense Cholesky does not clobber it either)
            info = sv.info()
            assert info["blockdiag_path"] == "batched-unpivoted" and info["blockdiag_block"] == -1


def test_damped_solve_against_oracle_and_dense_handle(ctx):
    B, mb, nb = 16, 128, 32
    J = make_bd(B, mb, nb, 7)
    D = J.toarray()                                        # 2048 x 512
    rng = np.random.default_rng(5)
    y = rng.standard_normal(B * mb)
    damp = 0.01 + rng.random(B * nb)
    x, nmul, _, _ = dev_solve(ctx, lsq.DeviceMatrix(ctx, J), y, damp)
    st, xo, nmul_o, _ = O.ldiv(O.CHOLESKY, O.Mat(dense=D), y, damp)
    assert st == 0 and nmul == nmul_o == 1
    xd, nmul_d, svd, _ = dev_solve(ctx, lsq.DeviceMatrix(ctx, D), y, damp)
    assert svd.info()["blockdiag_path"] is None
    print("damped 16x128x32: vs oracle %.3e, vs dense handle %.3e, vs numpy %.3e"
          % (rel_err(x, xo), rel_err(x, xd), rel_err(x, blocks_solve(J, y, damp))))
    assert rel_err(x, xo) <= SOLVE_RTOL
    assert rel_err(x, xd) <= SOLVE_RTOL
    assert rel_err(x, blocks_solve(J, y, damp)) <= SOLVE_RTOL


@pytest.mark.parametrize("B,mb,nb", [(16, 128, 32), (300, 257, 64), (300, 64, 8)])
def test_damped_solve_column_scaled(ctx, B, mb, nb):
    """J = V diag(s) (lsq_mat_set_colscale): multiplied out on the small handle, applied to G and r inside the solve on the
    sliced layouts of the big ones (nnz >= 2^20), never materialised there."""
    V = make_bd(B, mb, nb, 11)
    rng = np.random.default_rng(B + nb)
    s = 0.25 + rng.random(B * nb)
    Jd = lsq.DeviceMatrix(ctx, V)
    ds = lsq.DeviceVector(ctx, B * nb, s)
    Jd.set_colscale(ds)
    J = lsq.BlockDiagonal(B, mb, nb, data=V.data * np.repeat(s, mb))
    y = rng.standard_normal(B * mb)
    damp = 0.02 + rng.random(B * nb)
    x, _, _, _ = dev_solve(ctx, Jd, y, damp)
    assert rel_err(x, blocks_solve(J, y, damp)) <= SOLVE_RTOL
    if mb >= nb:
        x, _, _, _ = dev_solve(ctx, Jd, y)
        assert rel_err(x, blocks_solve(J, y)) <= SOLVE_RTOL
    Jd.set_colscale(None)
    x, _, _, _ = dev_solve(ctx, Jd, y, damp)
    assert rel_err(x, blocks_solve(V, y, damp)) <= SOLVE_RTOL


# ------------------------------------------------------------------------------------------ 3. undamped (Dogleg) solve
@pytest.mark.parametrize("B,mb,nb", [(16, 128, 32), (7, 64, 5), (300, 257, 64), (1, 64, 16), (300, 64, 17), (7, 257, 48), (7, 3, 1)])
def test_undamped_solve_full_rank(ctx, B, mb, nb):
    J = make_bd(B, mb, nb, 21)
    rng = np.random.default_rng(nb)
    y = rng.standard_normal(B * mb)
    x, nmul, sv, _ = dev_solve(ctx, lsq.DeviceMatrix(ctx, J), y)
    assert nmul == 1 and sv.info()["blockdiag_path"] == "batched-pivoted" and sv.info()["blockdiag_block"] == -1
    err = rel_err(x, blocks_solve(J, y))
    print("undamped nb=%d mb=%d B=%d rel err %.3e" % (nb, mb, B, err))
    assert err <= SOLVE_RTOL
    if (B, mb, nb) == (16, 128, 32):
        D = J.toarray()
        st, xo, nmul_o = O.ldiv(O.CHOLESKY, O.Mat(dense=D), y)
        assert st == 0 and nmul_o == 1
        assert rel_err(x, xo) <= SOLVE_RTOL
        xd, _, _, _ = dev_solve(ctx, lsq.DeviceMatrix(ctx, D), y)
        assert rel_err(x, xd) <= SOLVE_RTOL


def test_undamped_solve_and_rank_deficiency(ctx):
    """One duplicated column in block 11 -> RankDeficientException, the solver names block 11, the oracle's pivoted Cholesky
    refuses the stacked dense operand.  With the reference's tol = 0 the verdict on a duplicated column is the SIGN of the last
    pivot; so that it is not rounding noise the duplicated column is 64 ones over 64 zeros: its squared norm 64 is the
    largest diagonal entry (the other columns have norm ~1), so both copies are pivoted first in either pivot order; sqrt(64)
    = 8 and every quotient / product with it is exact, which leaves the second copy's pivot and its whole row of the factor
    EXACTLY zero in the oracle's left-looking and in the device's right-looking elimination alike."""
    B, mb, nb, bad = 16, 128, 32, 11
    J = make_bd(B, mb, nb, 7)
    col = np.zeros(mb)
    col[:64] = 1.0
    J.block(bad)[:, 4] = col
    J.block(bad)[:, 20] = col
    rng = np.random.default_rng(8)
    y = rng.standard_normal(B * mb)
    st = O.ldiv(O.CHOLESKY, O.Mat(dense=J.toarray()), y)[0]
    assert st == O.ERANK
    Jd = lsq.DeviceMatrix(ctx, J)
    sv = lsq.AllocatedSolver(Jd, lsq.Cholesky(), for_lm=False)
    with pytest.raises(lsq.RankDeficientException) as e:
        sv.ldiv_(lsq.DeviceVector(ctx, Jd.n), lsq.DeviceVector(ctx, Jd.m, y))
    assert e.value.status == lsq._lib.ERANK
    assert "RankDeficientException(%d)" % (B * nb - 1) in str(e.value)      # the stacked factorisation's rank
    info = sv.info()
    assert info["blockdiag_path"] == "batched-pivoted" and info["blockdiag_block"] == bad
    # the dense handle's pivoted solve of the stacked matrix refuses it too
    with pytest.raises(lsq.RankDeficientException):
        dev_solve(ctx, lsq.DeviceMatrix(ctx, J.toarray()), y)
    # mb < nb: the undamped normal matrix is singular by construction (an exactly zero column makes it exact)
    K = make_bd(7, 3, 5, 2)
    K.block(2)[:, 1] = 0.0
    with pytest.raises(lsq.RankDeficientException):
        dev_solve(ctx, lsq.DeviceMatrix(ctx, K), rng.standard_normal(21))
    # the solver is reusable after a refusal
    x, _, _, _ = dev_solve(ctx, lsq.DeviceMatrix(ctx, make_bd(B, mb, nb, 7)), y)
    assert np.all(np.isfinite(x))


# ------------------------------------------------------------------------------------------ 4. not positive definite
def test_not_positive_definite_reports_the_stacked_column(ctx):
    B, mb, nb = 16, 128, 32
    J = make_bd(B, mb, nb, 7)
    D = J.toarray()
    rng = np.random.default_rng(3)
    y = rng.standard_normal(B * mb)
    damp = 0.01 + rng.random(B * nb)
    for b, k in ((9, 1), (5, 3)):                     # 0-based column k of block b gets a negative diagonal entry
        damp[b * nb + k] = -(np.sum(J.block(b)[:, k] ** 2) + 10.0)
    expect = 5 * nb + 3 + 1                           # dpotrf's 1-based column in the LOWER of the two blocks
    assert O.ldiv(O.CHOLESKY, O.Mat(dense=D), y, damp)[0] == O.ENOTPD
    Jd = lsq.DeviceMatrix(ctx, J)
    sv = lsq.AllocatedSolver(Jd, lsq.Cholesky(), for_lm=True)
    with pytest.raises(lsq.PosDefException) as e:
        sv.ldiv_(lsq.DeviceVector(ctx, Jd.n), lsq.DeviceVector(ctx, Jd.m, y), lsq.DeviceVector(ctx, Jd.n, damp))
    assert e.value.status == lsq._lib.ENOTPD
    assert str(e.value).endswith("Cholesky failed at %d" % expect), str(e.value)
    assert sv.info()["blockdiag_block"] == 5
    with pytest.raises(lsq.PosDefException) as ed:
        dev_solve(ctx, lsq.DeviceMatrix(ctx, D), y, damp)
    assert str(ed.value) == str(e.value)
    # one wavefront per block (nb <= 16) reports the same way
    J2 = make_bd(7, 64, 5, 1)
    damp2 = np.full(35, 0.5)
    damp2[6 * 5 + 4] = -100.0
    damp2[3 * 5 + 2] = -100.0
    sv2 = lsq.AllocatedSolver(lsq.DeviceMatrix(ctx, J2), lsq.Cholesky(), for_lm=True)
    with pytest.raises(lsq.PosDefException) as e2:
        sv2.ldiv_(lsq.DeviceVector(ctx, 35), lsq.DeviceVector(ctx, 7 * 64, rng.standard_normal(7 * 64)), lsq.DeviceVector(ctx, 35, damp2))
    assert str(e2.value).endswith("Cholesky failed at %d" % (3 * 5 + 2 + 1)) and sv2.info()["blockdiag_block"] == 3


# ------------------------------------------------------------------------------------------ 5. refusals that must stay
def test_refusals(ctx):
    J = make_bd(4, 16, 8, 1)
    Jd = lsq.DeviceMatrix(ctx, J)
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.AllocatedSolver(Jd, lsq.QR(), for_lm=True)
    assert e.value.status == lsq._lib.EARG
    assert str(e.value) == "solver QR() is not available for sparse Jacobians. Choose between Cholesky() and LSMR()"
    # a plain CSC handle holding the very same pattern: no pattern sniffing
    Jc = lsq.DeviceMatrix(ctx, J.tocsc())
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.AllocatedSolver(Jc, lsq.Cholesky(), for_lm=True)
    assert e.value.status == lsq._lib.EARG
    assert str(e.value) == ("MethodError: no AbstractAllocatedSolver for Cholesky() with a sparse Jacobian "
                            "(dense_cholesky.jl:19 requires a StridedVecOrMat)")
    with pytest.raises(lsq.ArgumentError):
        lsq.AllocatedSolver(Jc, lsq.QR(), for_lm=False)
    # blocks wider than the 64 x 64 in-LDS factorisation
    J65 = lsq.DeviceMatrix(ctx, make_bd(2, 70, 65, 1))
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.AllocatedSolver(J65, lsq.Cholesky(), for_lm=True)
    assert e.value.status == lsq._lib.EARG and "64" in str(e.value) and "65" in str(e.value)
    lsq.AllocatedSolver(J65, lsq.LSMR(), for_lm=True)        # ... LSMR() takes it
    with pytest.raises(lsq.ArgumentError):
        lsq.optimize_(lsq.LeastSquaresProblem(x=np.zeros(32), f_=lambda o, x: None, g_=lambda J, x: None, J=J), lsq.Dogleg(lsq.QR()))
    # a solver allocated for one block shape refuses another handle
    sv = lsq.AllocatedSolver(Jd, lsq.Cholesky(), for_lm=True)
    other = lsq.DeviceMatrix(ctx, make_bd(2, 32, 16, 1))      # same m x n, other blocks
    sv.J = other
    with pytest.raises(lsq.DimensionMismatch):
        sv.ldiv_(lsq.DeviceVector(ctx, 32), lsq.DeviceVector(ctx, 64), lsq.DeviceVector(ctx, 32, np.ones(32)))


# ------------------------------------------------------------------------------------------ 6. / 7. trajectories
TRAJ = (16, 128, 32)
TRAJ_SEED = 7


def tanh_setup(B, mb, nb, seed):
    """The block-diagonal tanh problem r = A tanh(x) - b and its oracle twin on the STACKED DENSE Jacobian."""
    A = make_bd(B, mb, nb, seed)
    m, n = A.shape
    A3 = A.data.reshape((B, nb, mb))
    mv = lambda t: np.einsum("bjr,bj->br", A3, t.reshape((B, nb))).reshape(-1)
    _, b = lsq.synthetic.rhs_for(mv, m, n, seed)
    Ad = O.Mat(dense=A.toarray())
    Jo = O.Mat(dense=np.zeros((m, n)))
    f, g, ud, keep = O.tanh_model(Ad, b)
    return A, b, mv, (Jo, f, g, ud, keep)


def host_problem(A, b, mv):
    B, mb, nb = A.nblocks, A.mb, A.nb

    def f_(out, x):
        out[:] = mv(np.tanh(x)) - b

    def g_(J, x):                                           # the generic contract: g! overwrites J.data
        J.data[:] = A.data * np.repeat(1.0 - np.tanh(x) ** 2, mb)

    return lsq.LeastSquaresProblem(x=np.zeros(B * nb), y=np.zeros(B * mb), f_=f_, g_=g_, J=lsq.BlockDiagonal(B, mb, nb))


@pytest.mark.parametrize("opt", ["lm", "dogleg"])
def test_trajectory_matches_the_oracle_on_the_stacked_dense_jacobian(ctx, opt):
    """Device model (f! / g! on the device) on the block handle, LevenbergMarquardt(Cholesky()) / Dogleg(Cholesky()), against
    O.optimize(.., CHOLESKY, dense stacked J): same counts and flags, per-iteration iterates and ssr.  The oracle side was
    run on the CPU beforehand: it converges in 6 (LM) / 7 (Dogleg) iterations at seed 7, far below `iterations`."""
    B, mb, nb = TRAJ
    A, b, mv, (Jo, f, g, ud, keep) = tanh_setup(B, mb, nb, TRAJ_SEED)
    okind, ookind = (lsq._lib.LEVENBERG_MARQUARDT, O.LM) if opt == "lm" else (lsq._lib.DOGLEG, O.DOGLEG)
    ro = O.optimize(ookind, O.CHOLESKY, Jo, np.zeros(B * nb), f, g, ud=ud, iterations=50)
    assert ro.status == 0 and ro.converged and ro.iterations <= 12
    pr = lsq.synthetic.TanhProblem(B * mb, B * nb, seed=TRAJ_SEED, ctx=ctx, blockdiag=TRAJ)
    assert np.array_equal(pr.b, b) and np.array_equal(pr.A, A.data)
    pr.reset()
    rg = pr.optimize(okind, lsq._lib.CHOLESKY, trace=True, iterations=50)
    print(opt, "iterations", rg.iterations, ro.iterations, "ssr", rg.ssr, ro.ssr)
    assert rg.iterations == ro.iterations
    assert (rg.f_calls, rg.g_calls, rg.mul_calls) == (ro.f_calls, ro.g_calls, ro.mul_calls)
    assert (rg.converged, rg.x_converged, rg.f_converged, rg.g_converged) == (ro.converged, ro.x_converged, ro.f_converged, ro.g_converged)
    excused = compare_until_roundoff(rg, ro, ssr0=float(np.sum(b * b)))
    assert excused is None
    assert np.max(np.abs(rg.minimizer - ro.minimizer)) <= 1e-8 * max(1.0, np.max(np.abs(ro.minimizer)))
    # the generic contract: a host-side g! that writes J.data, through the public optimize_
    nls = host_problem(A, b, mv)
    Opt = lsq.LevenbergMarquardt if opt == "lm" else lsq.Dogleg
    rh = lsq.optimize_(nls, Opt(lsq.Cholesky()), full_trace=True, iterations=50, ctx=ctx)
    assert rh.iterations == ro.iterations and rh.converged
    assert (rh.f_calls, rh.g_calls, rh.mul_calls) == (ro.f_calls, ro.g_calls, ro.mul_calls)
    compare_until_roundoff(rh, ro, ssr0=float(np.sum(b * b)))
    assert np.max(np.abs(rh.minimizer - ro.minimizer)) <= 1e-8 * max(1.0, np.max(np.abs(ro.minimizer)))
    pr.close()


def test_trajectory_column_scaled_device_model(ctx):
    """The structured contract: device model + column scaling on the sliced layouts (8 blocks of 4096 x 32: nnz = 2^20, so
    J = A diag(s) is never multiplied out and the solve applies s to G and r) reaches the minimizer of the oracle run on the
    stacked dense Jacobian (32768 x 256: few, tall blocks keep the oracle's dense normal matrix affordable)."""
    B, mb, nb = 8, 4096, 32
    A, b, mv, (Jo, f, g, ud, keep) = tanh_setup(B, mb, nb, 9)
    ro = O.optimize(O.LM, O.CHOLESKY, Jo, np.zeros(B * nb), f, g, ud=ud, iterations=50, trace_x=False)
    assert ro.status == 0 and ro.converged
    pr = lsq.synthetic.TanhProblem(B * mb, B * nb, seed=9, ctx=ctx, blockdiag=(B, mb, nb))
    pr.reset()
    rg = pr.optimize(lsq._lib.LEVENBERG_MARQUARDT, lsq._lib.CHOLESKY, iterations=50)
    assert rg.converged and rg.iterations == ro.iterations
    assert np.max(np.abs(rg.minimizer - ro.minimizer)) <= 1e-8 * max(1.0, np.max(np.abs(ro.minimizer)))
    assert abs(rg.ssr - ro.ssr) <= 1e-9 * ro.ssr
    pr.close()


@pytest.mark.parametrize("opt", ["lm", "dogleg"])
def test_bounds(ctx, opt):
    """lower / upper on the trajectory problem: feasibility and equality with the oracle run.  With x_true ~ U(-1, 1) and the
    box [-0.7, 0.8] about a fifth of the bounds are active at the end.  The reference's clipped steps make this a long run
    (the oracle's LM has not met a tolerance after 100 iterations, its Dogleg needs 78): 25 iterations are compared, the
    convergence flags whatever they are."""
    B, mb, nb = TRAJ
    A, b, mv, (Jo, f, g, ud, keep) = tanh_setup(B, mb, nb, TRAJ_SEED)
    n = B * nb
    lower, upper = np.full(n, -0.7), np.full(n, 0.8)
    ookind = O.LM if opt == "lm" else O.DOGLEG
    ro = O.optimize(ookind, O.CHOLESKY, Jo, np.zeros(n), f, g, ud=ud, iterations=25, lower=lower, upper=upper)
    assert ro.status == 0
    nls = host_problem(A, b, mv)
    Opt = lsq.LevenbergMarquardt if opt == "lm" else lsq.Dogleg
    rg = lsq.optimize_(nls, Opt(lsq.Cholesky()), full_trace=True, iterations=25, lower=lower, upper=upper, ctx=ctx)
    assert np.all(rg.minimizer >= lower) and np.all(rg.minimizer <= upper)
    assert np.all(rg.trace["x"] >= lower) and np.all(rg.trace["x"] <= upper)          # every iterate is feasible
    assert np.sum(rg.minimizer == lower) + np.sum(rg.minimizer == upper) > 0        # some bounds are active
    assert rg.iterations == ro.iterations
    assert (rg.converged, rg.x_converged, rg.f_converged, rg.g_converged) == (ro.converged, ro.x_converged, ro.f_converged, ro.g_converged)
    assert (rg.f_calls, rg.g_calls, rg.mul_calls) == (ro.f_calls, ro.g_calls, ro.mul_calls)
    compare_until_roundoff(rg, ro, ssr0=float(np.sum(b * b)))
    assert np.max(np.abs(rg.minimizer - ro.minimizer)) <= 1e-8 * max(1.0, np.max(np.abs(ro.minimizer)))
    assert np.array_equal(rg.minimizer == lower, ro.minimizer == lower) and np.array_equal(rg.minimizer == upper, ro.minimizer == upper)


# ------------------------------------------------------------------------------------------ 8. at scale
def test_at_scale_against_lsmr_on_the_plain_csc_handle(ctx):
    """B = 4096 blocks of 256 x 16 (1 048 576 x 65 536, 16.8 M values): no dense comparison exists.  LM(Cholesky()) on the
    block handle against LM(LSMR()) on a plain CSC handle of the same matrix.  Both converge.  LSMR's inner solves stop at
    btol = 0.5 (iterative_lsmr.jl:238-259), so the paths differ; both runs stop on the outer x_tol = f_tol = g_tol = 1e-8
    (the same for the two solvers: that is the looser -- and only -- stopping tolerance in play), and a run that has stopped
    on one of them is within the step / gradient it stopped on of the minimizer; on this problem (J'J ~ 0.4 I .. I at the
    solution) 1e-8 in the gradient or in the last step bounds the distance to the minimizer by ~1e-7: minimizers are compared
    to 1e-6, final ssr to 1e-8 relative."""
    B, mb, nb = 4096, 256, 16
    m, n = B * mb, B * nb
    pr = lsq.synthetic.TanhProblem(m, n, seed=4, ctx=ctx, blockdiag=(B, mb, nb))
    # per-block spot check of a first LM step: at x0 = 0, J = A and f = -b; damping as levenberg_marquardt.jl:82-86 forms it
    A = lsq.BlockDiagonal(B, mb, nb, data=pr.A)
    Jd = lsq.DeviceMatrix(ctx, A)
    cs = lsq.colsumabs2_(lsq.DeviceVector(ctx, n), Jd).get()
    damp = np.clip(cs, 1e-6, 1e32) / 10.0                      # levenberg_marquardt.jl:82-86 with Delta = 10
    f0 = -pr.b
    x, nmul, _, _ = dev_solve(ctx, Jd, f0, damp)
    rng = np.random.default_rng(0)
    for blk in rng.choice(B, 64, replace=False):
        Ab = A.block(blk)
        ref = np.linalg.solve(Ab.T @ Ab + np.diag(damp[blk * nb:(blk + 1) * nb]), Ab.T @ f0[blk * mb:(blk + 1) * mb])
        assert rel_err(x[blk * nb:(blk + 1) * nb], ref) <= SOLVE_RTOL, blk
    Jd.free()
    pr.reset()
    rc = pr.optimize(lsq._lib.LEVENBERG_MARQUARDT, lsq._lib.CHOLESKY, iterations=50)
    assert rc.converged and rc.iterations <= 15
    # the parent's only way to run it: the same matrix as a plain CSC handle, LSMR
    S = A.tocsc()
    pl = lsq.synthetic.TanhProblem(m, n, sparse=True, seed=4, ctx=ctx, inputs=(S.indptr.astype(np.int32), S.indices.astype(np.int32), pr.A),
                                   b=pr.b)
    pl.reset()
    rl = pl.optimize(lsq._lib.LEVENBERG_MARQUARDT, lsq._lib.LSMR, iterations=50)
    assert rl.converged
    print("at scale: Cholesky %d iterations ssr %.12e %.4fs | LSMR %d outer %d inner ssr %.12e %.4fs | max|dx| %.3e"
          % (rc.iterations, rc.ssr, rc.seconds, rl.iterations, rl.lsmr_iterations, rl.ssr, rl.seconds,
             np.max(np.abs(rc.minimizer - rl.minimizer))))
    assert np.max(np.abs(rc.minimizer - rl.minimizer)) <= 1e-6 * max(1.0, np.max(np.abs(rl.minimizer)))
    assert abs(rc.ssr - rl.ssr) <= 1e-8 * rl.ssr
    pr.close()
    pl.close()


# ------------------------------------------------------------------------------------------ 9. debug modes / determinism
def test_serial_mode_and_repeatability(ctx):
    """debug_set(serial=1): same kernels, same arithmetic -> bit-identical; two runs of the same solve are bit-identical (no
    floating-point atomics: the words shared between blocks are integers)."""
    outs = {}
    for B, mb, nb in ((300, 257, 48), (300, 64, 8)):
        J = make_bd(B, mb, nb, 5)
        Jd = lsq.DeviceMatrix(ctx, J)
        rng = np.random.default_rng(1)
        y = rng.standard_normal(B * mb)
        damp = 0.1 + rng.random(B * nb)
        for damped in (True, False):
            runs = [dev_solve(ctx, Jd, y, damp if damped else None)[0] for _ in range(2)]
            assert np.array_equal(runs[0], runs[1])
            outs[(B, mb, nb, damped)] = (Jd, y, damp, runs[0])
    traj = {}
    for serial in (0, 1):
        lsq.debug_set(serial=serial)
        try:
            for key, (Jd, y, damp, ref) in outs.items():
                x = dev_solve(ctx, Jd, y, damp if key[3] else None)[0]
                assert np.array_equal(x, ref), (serial, key)
            for okind in (lsq._lib.LEVENBERG_MARQUARDT, lsq._lib.DOGLEG):
                pr = lsq.synthetic.TanhProblem(TRAJ[0] * TRAJ[1], TRAJ[0] * TRAJ[2], seed=TRAJ_SEED, ctx=ctx, blockdiag=TRAJ)
                pr.reset()
                r = pr.optimize(okind, lsq._lib.CHOLESKY, trace=True, iterations=50)
                traj[(serial, okind)] = (r.iterations, r.ssr, r.minimizer.copy(), r.trace["x"].copy())
                pr.close()
        finally:
            lsq.debug_set(serial=0)
    for okind in (lsq._lib.LEVENBERG_MARQUARDT, lsq._lib.DOGLEG):
        a, b = traj[(0, okind)], traj[(1, okind)]
        assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
