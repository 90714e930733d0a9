"""Bordered block-diagonal Jacobians J = [blkdiag(J_1 .. J_B) | C] on the device: the handle (lsq_blockdiag_bordered_create:
a CSC handle that knows its shape) and LevenbergMarquardt's Cholesky() on it (lsq_bordered.hip: eliminate the locals block by
block, factor the ng x ng Schur complement, back-substitute) against numpy on the dense normal equations, the oracle on the
STACKED dense matrix and the dense handle's own Cholesky() on the device.

Tolerances are the project's (tests/gpu_common.py), as tests/test_c_gpu_blockdiag.py uses them: kernels 1e-12 * scale, one
direct solve rel 1e-9, trajectories through compare_until_roundoff with its defaults.  Operands: the library's generator
(blocks N(0,1)/sqrt(mb), border N(0,1)/sqrt(m)), which is well conditioned."""
import ctypes as C

import numpy as np
import pytest

from gpu_common import compare_until_roundoff, lsq
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SOLVE_RTOL = 1e-9        # gpu_common: one direct solve
KERNEL_TOL = 1e-12       # gpu_common: kernels, times the scale of the result

DOGLEG_TEXT = ("Dogleg(Cholesky()) is not available on a bordered block-diagonal Jacobian: the reference's pivoted "
               "factorisation orders local and shared columns together, which does not split into blocks. "
               "Use LevenbergMarquardt(Cholesky()) or LSMR()")


def make_bb(B, mb, nb, ng, seed):
    return lsq.BorderedBlockDiagonal(B, mb, nb, ng, data=lsq.synthetic.bordered_inputs(B, mb, nb, ng, seed))


DENSE_REF_MAX_N = 2048


def dense_solve(J, y, damp):
    """numpy.linalg.solve on the normal equations (J'J + D) x = J'y of the stacked matrix.  Up to n = 2048 columns on the
    dense toarray(), as written.  Beyond that the dense normal matrix does not fit a test of a few seconds (300 blocks of 63
    columns: 18901^2 doubles, 2e12 flops), so the SAME equations are solved by numpy.linalg.solve block by block: the arrowhead
    system reduced to its ng x ng Schur complement.  test_reference_block_elimination_is_the_dense_solve holds the two forms
    of the reference to 1e-12 of each other where both can be formed."""
    if J.shape[1] <= DENSE_REF_MAX_N:
        D = J.toarray()
        return np.linalg.solve(D.T @ D + np.diag(damp), D.T @ y)
    return block_solve(J, y, damp)


def block_solve(J, y, damp):
    B, mb, nb, ng = J.nblocks, J.mb, J.nb, J.ng
    S = J.border.T @ J.border + np.diag(damp[B * nb:])
    rg = J.border.T @ y
    keep = []
    for b in range(B):
        A, Cb, yb = J.block(b), J.border_block(b), y[b * mb:(b + 1) * mb]
        G = A.T @ A + np.diag(damp[b * nb:(b + 1) * nb])
        W = np.linalg.solve(G, np.column_stack([A.T @ Cb, A.T @ yb]))      # inv(G) [A'C_b, A'y_b]
        S -= (A.T @ Cb).T @ W[:, :ng]
        rg -= (A.T @ Cb).T @ W[:, ng]
        keep.append(W)
    xg = np.linalg.solve(S, rg)
    return np.concatenate([W[:, ng] - W[:, :ng] @ xg for W in keep] + [xg])


def rel_err(x, ref):
    return np.linalg.norm(x - ref) / np.linalg.norm(ref)


def test_reference_block_elimination_is_the_dense_solve(ctx):
    for B, mb, nb, ng in ((7, 64, 16, 17), (16, 128, 24, 8), (30, 40, 5, 60)):
        J = make_bb(B, mb, nb, ng, 9)
        rng = np.random.default_rng(B)
        y, damp = rng.standard_normal(B * mb), 0.05 + rng.random(B * nb + ng)
        assert J.shape[1] <= DENSE_REF_MAX_N
        assert rel_err(block_solve(J, y, damp), dense_solve(J, y, damp)) <= 1e-12


def dev_solve(ctx, Jd, y, damp, sv=None):
    sv = sv or lsq.AllocatedSolver(Jd, lsq.Cholesky(), for_lm=True)
    dx = lsq.DeviceVector(ctx, Jd.n)
    dd = lsq.DeviceVector(ctx, Jd.n, damp)
    _, nmul = sv.ldiv_(dx, lsq.DeviceVector(ctx, Jd.m, y), dd)
    return dx.get(), nmul, sv, dd


# ------------------------------------------------------------------------------------------ 1. the handle is a CSC handle
@pytest.mark.parametrize("B,mb,nb,ng", [(7, 3, 5, 2), (16, 128, 32, 8), (300, 257, 17, 1)])
def test_handle_is_a_csc_handle(ctx, B, mb, nb, ng):
    J = make_bb(B, mb, nb, ng, 3)
    Jd = lsq.DeviceMatrix(ctx, J)
    assert Jd.bordered_info() == (B, mb, nb, ng) and Jd.blockdiag_info() == (0, 0, 0)
    assert (Jd.m, Jd.n, Jd.nnz) == (B * mb, B * nb + ng, B * mb * (nb + ng))
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
    # handles that are not bordered say so
    assert lsq.DeviceMatrix(ctx, lsq.BlockDiagonal(B, mb, nb)).bordered_info() == (0, 0, 0, 0)
    assert lsq.DeviceMatrix(ctx, np.zeros((4, 3))).bordered_info() == (0, 0, 0, 0)


# ------------------------------------------------------------------------------------------ 2. one damped solve
@pytest.mark.parametrize("nb,ng", [(1, 1), (5, 3), (8, 8), (15, 1), (1, 16), (16, 17), (40, 8), (1, 63), (63, 1), (32, 32)])
def test_damped_solve_every_shape(ctx, nb, ng):
    """lsq_ldiv_damped, every kernel branch: one wavefront per block (nb + ng = 2, 8, 16) and one workgroup per block with 2,
    3 and 4 tile rows, the Schur part the smallest and the largest share; mb below one chunk (the damping makes it solvable),
    exactly two chunks, a ragged ninth chunk; a single block, a grid that ends inside a workgroup of four (7), 300 blocks
    (more than one group of the contribution sum)."""
    for mb, B in ((3, 1), (64, 7), (257, 300)):
        J = make_bb(B, mb, nb, ng, 1000 * nb + 10 * ng + mb + B)
        n = B * nb + ng
        rng = np.random.default_rng(nb * mb + B + ng)
        y = rng.standard_normal(B * mb)
        damp = 0.05 + rng.random(n)
        x, nmul, sv, dd = dev_solve(ctx, lsq.DeviceMatrix(ctx, J), y, damp)
        err = rel_err(x, dense_solve(J, y, damp))
        print("damped nb=%d ng=%d mb=%d B=%d rel err %.3e" % (nb, ng, mb, B, err))
        assert err <= SOLVE_RTOL, (nb, ng, mb, B, err)
        assert nmul == 1
        assert np.array_equal(dd.get(), damp)              # not clobbered
        info = sv.info()
        assert info["blockdiag_path"] == "bordered-schur" and info["blockdiag_block"] == -1


# ------------------------------------------------------------------------------------------ 3. oracle and dense handle
def test_damped_solve_against_oracle_and_dense_handle(ctx):
    B, mb, nb, ng = 16, 128, 24, 8
    J = make_bb(B, mb, nb, ng, 7)
    D = J.toarray()                                        # 2048 x 392
    rng = np.random.default_rng(5)
    y = rng.standard_normal(B * mb)
    damp = 0.01 + rng.random(B * nb + ng)
    x, nmul, _, _ = dev_solve(ctx, lsq.DeviceMatrix(ctx, J), y, damp)
    st, xo, nmul_o, _ = O.ldiv(O.CHOLESKY, O.Mat(dense=D), y, damp)
    assert st == 0 and nmul == nmul_o == 1
    xd, nmul_d, svd, _ = dev_solve(ctx, lsq.DeviceMatrix(ctx, D), y, damp)
    assert svd.info()["blockdiag_path"] is None
    print("damped 16x128x24+8: vs oracle %.3e, vs dense handle %.3e, vs numpy %.3e"
          % (rel_err(x, xo), rel_err(x, xd), rel_err(x, dense_solve(J, y, damp))))
    assert rel_err(x, xo) <= SOLVE_RTOL
    assert rel_err(x, xd) <= SOLVE_RTOL


# ------------------------------------------------------------------------------------------ 4. column-scaled handle
@pytest.mark.parametrize("B,mb,nb,ng", [(16, 128, 24, 8), (300, 64, 6, 2), (300, 257, 17, 5)])
def test_damped_solve_column_scaled(ctx, B, mb, nb, ng):
    """J = V diag(s) (lsq_mat_set_colscale), s of length n: the ng border factors included.  The first two shapes are
    multiplied out by the handle; the third (nnz >= 2^20: sliced layouts) is never multiplied out -- the solve applies s to G
    and r itself."""
    V = make_bb(B, mb, nb, ng, 11)
    n, m = B * nb + ng, B * mb
    rng = np.random.default_rng(B + nb)
    y = rng.standard_normal(m)
    damp = 0.02 + rng.random(n)
    Jd = lsq.DeviceMatrix(ctx, V)
    s = 0.25 + rng.random(n)
    ds = lsq.DeviceVector(ctx, n, s)
    Jd.set_colscale(ds)
    sv = None
    for round_ in range(2):
        J = lsq.BorderedBlockDiagonal(B, mb, nb, ng, data=V.data * np.concatenate([np.repeat(s[:B * nb], mb), np.repeat(s[B * nb:], m)]))
        x, _, sv, _ = dev_solve(ctx, Jd, y, damp, sv)
        err = rel_err(x, dense_solve(J, y, damp))
        print("column-scaled B=%d round %d rel err %.3e" % (B, round_, err))
        assert err <= SOLVE_RTOL
        s = 0.25 + rng.random(n)                           # change s in place and say so
        ds.set(s)
        Jd.colscale_changed()
    Jd.set_colscale(None)
    x, _, _, _ = dev_solve(ctx, Jd, y, damp, sv)
    assert rel_err(x, dense_solve(V, y, damp)) <= SOLVE_RTOL


# ------------------------------------------------------------------------------------------ 5. not positive definite
@pytest.mark.parametrize("mb,nb,ng", [(64, 20, 6), (64, 5, 3)])
def test_not_positive_definite_reports_the_stacked_column(ctx, mb, nb, ng):
    """PosDefException parity with operands whose failing pivot is EXACT: an all-zero column with zero damping has exact zeros
    in its row of J'J, hence in its column of the factor, and its pivot is exactly 0 - 0 in any elimination order."""
    B = 5
    n, m = B * nb + ng, B * mb
    rng = np.random.default_rng(3)
    y = rng.standard_normal(m)
    kl, kg = 3, 1                                         # 0-based local column (of block 2) / border column
    good = make_bb(B, mb, nb, ng, 7)
    Jd_good = lsq.DeviceMatrix(ctx, good)
    damp_good = 0.01 + rng.random(n)
    for case in ("local", "border", "both"):
        J = make_bb(B, mb, nb, ng, 7)
        damp = damp_good.copy()
        if case in ("local", "both"):
            J.block(2)[:, kl] = 0.0
            damp[2 * nb + kl] = 0.0
        if case in ("border", "both"):
            J.border[:, kg] = 0.0
            damp[B * nb + kg] = 0.0
        expect, block = (B * nb + kg + 1, B) if case == "border" else (2 * nb + kl + 1, 2)
        D = J.toarray()
        assert O.ldiv(O.CHOLESKY, O.Mat(dense=D), y, damp)[0] == O.ENOTPD
        assert O.potrf_upper(D.T @ D + np.diag(damp))[0] == expect        # the oracle's dpotrf on the stacked normal matrix
        Jd = lsq.DeviceMatrix(ctx, J)
        sv = lsq.AllocatedSolver(Jd, lsq.Cholesky(), for_lm=True)
        with pytest.raises(lsq.PosDefException) as e:
            sv.ldiv_(lsq.DeviceVector(ctx, n), lsq.DeviceVector(ctx, m, y), lsq.DeviceVector(ctx, n, damp))
        assert e.value.status == lsq._lib.ENOTPD
        assert str(e.value) == "PosDefException: matrix is not positive definite; Cholesky failed at %d" % expect, (case, str(e.value))
        info = sv.info()
        assert info["blockdiag_path"] == "bordered-schur" and info["blockdiag_block"] == block, (case, info)
        with pytest.raises(lsq.PosDefException) as ed:                    # the dense handle says the same
            dense_sv = lsq.AllocatedSolver(lsq.DeviceMatrix(ctx, D), lsq.Cholesky(), for_lm=True)
            dense_sv.ldiv_(lsq.DeviceVector(ctx, n), lsq.DeviceVector(ctx, m, y), lsq.DeviceVector(ctx, n, damp))
        assert str(ed.value) == str(e.value)
        # a following well-posed solve on the same solver is correct
        sv.J = Jd_good
        x, _, _, _ = dev_solve(ctx, Jd_good, y, damp_good, sv)
        assert rel_err(x, dense_solve(good, y, damp_good)) <= SOLVE_RTOL
        assert sv.info()["blockdiag_block"] == -1


# ------------------------------------------------------------------------------------------ 6. determinism
def test_repeatability_and_serial_mode(ctx):
    B, mb, nb, ng = 300, 257, 17, 5
    J = make_bb(B, mb, nb, ng, 5)
    Jd = lsq.DeviceMatrix(ctx, J)
    rng = np.random.default_rng(1)
    y = rng.standard_normal(B * mb)
    damp = 0.1 + rng.random(B * nb + ng)
    runs = [dev_solve(ctx, Jd, y, damp)[0] for _ in range(2)]
    assert np.array_equal(runs[0], runs[1])
    lsq.debug_set(serial=1)
    try:
        x = dev_solve(ctx, Jd, y, damp)[0]
    finally:
        lsq.debug_set(serial=0)
    assert np.array_equal(x, runs[0])
    assert rel_err(x, dense_solve(J, y, damp)) <= SOLVE_RTOL


# ------------------------------------------------------------------------------------------ 7. the LM loop
FIT = (6, 40, 2, 2)


def exp_fit():
    """A separable global fit: data set b is a_b exp(-k1 t) + o_b exp(-k2 t) + noise on 40 points; the amplitudes a_b, o_b
    are local, the two decay rates are shared.  x = (a_0, o_0, a_1, o_1, .., k1, k2)."""
    B, mb, nb, ng = FIT
    t = np.linspace(0.0, 6.0, mb)
    rng = np.random.default_rng(42)
    a, o = 1.0 + rng.random(B), 0.5 + rng.random(B)
    k = np.array([1.5, 0.15])
    data = (a[:, None] * np.exp(-k[0] * t) + o[:, None] * np.exp(-k[1] * t) + 1e-3 * rng.standard_normal((B, mb))).reshape(-1)
    x0 = np.concatenate([np.tile([1.0, 1.0], B), [1.0, 0.3]])

    def parts(x):
        loc = x[:B * nb].reshape((B, nb))
        e1, e2 = np.exp(-x[B * nb] * t), np.exp(-x[B * nb + 1] * t)
        return loc, e1, e2

    def f_(out, x):
        loc, e1, e2 = parts(x)
        out[:] = (loc[:, :1] * e1 + loc[:, 1:] * e2).reshape(-1) - data

    def fill(J, x):                                        # J: a BorderedBlockDiagonal (views into J.data)
        loc, e1, e2 = parts(x)
        for b in range(B):
            blk = J.block(b)
            blk[:, 0], blk[:, 1] = e1, e2
            cb = J.border_block(b)
            cb[:, 0], cb[:, 1] = -loc[b, 0] * t * e1, -loc[b, 1] * t * e2

    def g_dense_flat(jflat, x):                            # the oracle's dense stacked Jacobian, column-major
        T = lsq.BorderedBlockDiagonal(B, mb, nb, ng)
        fill(T, x)
        jflat[:] = T.toarray().reshape(-1, order="F")

    return data, x0, f_, fill, g_dense_flat


def exp_problem(x0, f_, fill):
    B, mb, nb, ng = FIT
    return lsq.LeastSquaresProblem(x=x0.copy(), y=np.zeros(B * mb), f_=f_, g_=fill, J=lsq.BorderedBlockDiagonal(B, mb, nb, ng))


@pytest.mark.parametrize("bounded", [False, True])
def test_lm_trajectory_matches_the_oracle_on_the_stacked_dense_jacobian(ctx, bounded):
    B, mb, nb, ng = FIT
    m, n = B * mb, B * nb + ng
    data, x0, f_, fill, g_flat = exp_fit()
    kw = {}
    if bounded:                                            # active at the end: the shared k1 (true 1.5) and the local a_2 (true < 2)
        lower, upper = np.full(n, -np.inf), np.full(n, np.inf)
        upper[B * nb] = 1.2
        lower[2 * nb] = 2.5
        x0 = x0.copy()
        x0[2 * nb] = 3.0
        kw = dict(lower=lower, upper=upper)
    ssr0 = float(np.sum(_residual(f_, x0, m) ** 2))
    # (the reference's clipped steps make the bounded run a long one -- the oracle has met no tolerance after 60 iterations:
    #  25 are compared, the convergence flags whatever they are, as in test_c_gpu_blockdiag.py::test_bounds)
    its = 25 if bounded else 60
    ro = O.optimize(O.LM, O.CHOLESKY, O.Mat(dense=np.zeros((m, n))), x0, f_, g_flat, iterations=its, **kw)
    assert ro.status == 0
    rg = lsq.optimize_(exp_problem(x0, f_, fill), lsq.LevenbergMarquardt(lsq.Cholesky()), full_trace=True, iterations=its, ctx=ctx, **kw)
    print("bounded" if bounded else "free", "iterations", rg.iterations, ro.iterations, "ssr", rg.ssr, ro.ssr)
    assert rg.iterations == ro.iterations
    assert (rg.f_calls, rg.g_calls, rg.mul_calls) == (ro.f_calls, ro.g_calls, ro.mul_calls)
    assert (rg.converged, rg.x_converged, rg.f_converged, rg.g_converged) == (ro.converged, ro.x_converged, ro.f_converged, ro.g_converged)
    compare_until_roundoff(rg, ro, ssr0=ssr0)
    assert np.max(np.abs(rg.minimizer - ro.minimizer)) <= 1e-8 * max(1.0, np.max(np.abs(ro.minimizer)))
    if bounded:
        assert ro.minimizer[B * nb] == 1.2 and ro.minimizer[2 * nb] == 2.5
        assert rg.minimizer[B * nb] == 1.2 and rg.minimizer[2 * nb] == 2.5
        assert np.all(rg.trace["x"] >= lower) and np.all(rg.trace["x"] <= upper)
    else:
        assert ro.converged
        # Cholesky() without an optimizer means LevenbergMarquardt on this container
        rd = lsq.optimize_(exp_problem(x0, f_, fill), lsq.api.AbstractOptimizer(lsq.Cholesky()), iterations=60, ctx=ctx)
        assert rd.optimizer == "LevenbergMarquardt" and rd.iterations == rg.iterations and np.array_equal(rd.minimizer, rg.minimizer)
        # LevenbergMarquardt(LSMR()) on the same container reaches the same minimizer: the tolerance of the block-diagonal
        # LSMR-vs-Cholesky comparison (test_c_gpu_blockdiag.py: minimizers 1e-6, final ssr 1e-8 relative)
        rl = lsq.optimize_(exp_problem(x0, f_, fill), lsq.LevenbergMarquardt(lsq.LSMR()), iterations=200, ctx=ctx)
        assert rl.converged
        print("LSMR: %d iterations, max|dx| %.3e, ssr %.12e vs %.12e" % (rl.iterations, np.max(np.abs(rl.minimizer - rg.minimizer)), rl.ssr, rg.ssr))
        assert np.max(np.abs(rl.minimizer - rg.minimizer)) <= 1e-6 * max(1.0, np.max(np.abs(rg.minimizer)))
        assert abs(rl.ssr - rg.ssr) <= 1e-8 * rg.ssr


def _residual(f_, x, m):
    out = np.zeros(m)
    f_(out, x)
    return out


# ------------------------------------------------------------------------------------------ 8. refusals through the C ABI
def test_refusals_through_the_c_abi(ctx):
    L = lsq.lib()
    J = make_bb(4, 16, 8, 3, 1)
    Jd = lsq.DeviceMatrix(ctx, J)
    n, m = Jd.n, Jd.m
    rng = np.random.default_rng(2)
    y, damp = rng.standard_normal(m), 0.1 + rng.random(n)

    def still_works():
        x, _, _, _ = dev_solve(ctx, Jd, y, damp)
        assert rel_err(x, dense_solve(J, y, damp)) <= SOLVE_RTOL

    # nb + ng = 65
    J65 = lsq.DeviceMatrix(ctx, make_bb(2, 70, 60, 5, 1))
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.AllocatedSolver(J65, lsq.Cholesky(), for_lm=True)
    assert e.value.status == lsq._lib.EARG
    assert "nb + ng <= 64" in str(e.value) and "nb = 60, ng = 5" in str(e.value) and "LSMR()" in str(e.value)
    lsq.AllocatedSolver(J65, lsq.LSMR(), for_lm=True)        # ... LSMR() takes it
    still_works()
    # for_lm = 0
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.AllocatedSolver(Jd, lsq.Cholesky(), for_lm=False)
    assert e.value.status == lsq._lib.EARG and str(e.value) == DOGLEG_TEXT
    still_works()
    # lsq_ldiv on a solver allocated for LM
    sv = lsq.AllocatedSolver(Jd, lsq.Cholesky(), for_lm=True)
    with pytest.raises(lsq.ArgumentError) as e:
        sv.ldiv_(lsq.DeviceVector(ctx, n), lsq.DeviceVector(ctx, m, y))
    assert e.value.status == lsq._lib.EARG and str(e.value) == DOGLEG_TEXT
    x, _, _, _ = dev_solve(ctx, Jd, y, damp, sv)
    assert rel_err(x, dense_solve(J, y, damp)) <= SOLVE_RTOL
    # LSQ_BLOCK_QR and LSQ_QR: the code that refuses every handle without a block shape / every sparse handle
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.AllocatedSolver(Jd, lsq.BlockQR(), for_lm=True)
    assert e.value.status == lsq._lib.EARG and "BlockQR() needs a block-diagonal Jacobian" in str(e.value)
    still_works()
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.AllocatedSolver(Jd, lsq.QR(), for_lm=True)
    assert str(e.value) == "solver QR() is not available for sparse Jacobians. Choose between Cholesky() and LSMR()"
    still_works()
    # lsq_optimize_batched
    F = lsq._lib.F_CALLBACK(lambda d_out, d_x, user: 0)
    G = lsq._lib.G_CALLBACK(lambda Jh, d_x, user: 0)
    st, _ = lsq.api._run_native_batched(ctx, lsq._lib.LEVENBERG_MARQUARDT, lsq._lib.CHOLESKY, Jd.h, (4, 16, 8),
                                        lsq.DeviceVector(ctx, n), lsq.DeviceVector(ctx, m), F, G, None, 1e-8, 1e-8, 1e-8, 5, None,
                                        None, None, False, "LevenbergMarquardt")
    assert st == lsq._lib.EARG
    assert "the Jacobian is not block-diagonal" in L.lsq_last_error().decode()
    still_works()
    # lsq_optimize with Dogleg + Cholesky: the loop's own solver creation takes the same refusal
    st, _, _ = lsq.api._run_native(ctx, lsq._lib.DOGLEG, lsq._lib.CHOLESKY, Jd, lsq.DeviceVector(ctx, n), lsq.DeviceVector(ctx, m),
                                   F, G, None, 1e-8, 1e-8, 1e-8, 5, None, None, None, False, n)
    assert st == lsq._lib.EARG and L.lsq_last_error().decode() == DOGLEG_TEXT
    still_works()
    # the create call's own argument checks
    h = C.c_void_p()
    for args in ((0, 3, 2, 1), (2, 0, 2, 1), (2, 3, 0, 1), (2, 3, 2, 0), (1 << 20, 1 << 12, 2, 1)):
        assert L.lsq_blockdiag_bordered_create(ctx.h, *args, C.byref(h)) == lsq._lib.EDIM, args
