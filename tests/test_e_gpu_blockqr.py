"""BlockQR(): column-pivoted QR per block of a block-diagonal Jacobian (lsq_blockqr.hip).

The reference throughout is the oracle on every block ALONE: O.qr_solve(J_b, y_b) (dense_qr.jl:30-42, rcond = min(mb, nb) eps)
and O.ldiv(O.QR, J_b, y_b, damp_b) (dense_qr.jl:56-88, rcond = nb eps), with the tolerances of test_b_gpu_kernels.py::
test_ldiv_qr: undamped rtol 1e-8 / atol 1e-10, damped rtol 1e-9 / atol 1e-12, ranks exactly equal."""
import ctypes as C

import numpy as np
import pytest

from gpu_common import compare_until_roundoff, lsq
from oracle import oracle as O
from test_c_gpu_blockdiag import host_problem as stacked_host_problem, tanh_setup
from test_d_gpu_batched import host_problem as batched_host_problem, plain_problem, same_counts

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
NBS = [1, 5, 16, 17, 33, 64]
MBS = [3, 40, 257]


def make_bd(B, mb, nb, seed):
    return lsq.BlockDiagonal(B, mb, nb, data=lsq.synthetic.blockdiag_inputs(B, mb, nb, seed))


def bq_solve(ctx, Jd, y, damp=None):
    sv = lsq.AllocatedSolver(Jd, lsq.BlockQR(), for_lm=damp is not None)
    dx = lsq.DeviceVector(ctx, Jd.n)
    dy = lsq.DeviceVector(ctx, Jd.m, y)
    dd = lsq.DeviceVector(ctx, Jd.n, damp) if damp is not None else None
    _, nmul = sv.ldiv_(dx, dy, dd)
    return dx.get(), nmul, sv, dy, dd


def oracle_blocks(J, y, damp=None):
    """(x, ranks) of the per-block oracle solves."""
    B, mb, nb = J.nblocks, J.mb, J.nb
    x, ranks = np.zeros(B * nb), np.zeros(B, dtype=np.int64)
    for b in range(B):
        Jb, yb = np.array(J.block(b), order="F"), y[b * mb:(b + 1) * mb]
        if damp is None:
            xb, rk, *_ = O.qr_solve(Jb, yb)
        else:
            db = damp[b * nb:(b + 1) * nb]
            st, xb, nmul, _ = O.ldiv(O.QR, O.Mat(dense=Jb), yb, db)
            assert st == 0 and nmul == 1
            # the same factorisation once more for its rank (orc_ldiv_qr_damped keeps it to itself)
            _, rk, *_ = O.qr_solve(np.vstack([Jb, np.diag(np.sqrt(db))]), np.concatenate([yb, np.zeros(nb)]), rcond=nb * EPS)
        x[b * nb:(b + 1) * nb], ranks[b] = xb, rk
    return x, ranks


def assert_blocks_close(x, ref, nb, rtol, atol, label):
    for b in range(len(ref) // nb):
        xb, rb = x[b * nb:(b + 1) * nb], ref[b * nb:(b + 1) * nb]
        assert np.allclose(xb, rb, rtol=rtol, atol=atol), (label, b, float(np.max(np.abs(xb - rb))))


# ------------------------------------------------------------------------------------------ 1. undamped, every branch
@pytest.mark.parametrize("nb", NBS)
def test_undamped_solve_every_branch(ctx, nb):
    """One wavefront per block (nb <= 16) and one workgroup per block; one short chunk, one long chunk, a ragged fifth chunk;
    mb < nb (rank mb, minimum norm); a single block, a grid that ends inside a workgroup of four, 300 blocks."""
    for mb in MBS:
        for B in (1, 7, 300):
            J = make_bd(B, mb, nb, 2000 * nb + mb + B)
            y = np.random.default_rng(nb * mb + B).standard_normal(B * mb)
            x, nmul, sv, dy, _ = bq_solve(ctx, lsq.DeviceMatrix(ctx, J), y)
            ref, ranks = oracle_blocks(J, y)
            info = sv.info()
            assert np.all(ranks == min(mb, nb))
            assert np.array_equal(info["block_ranks"], ranks), (nb, mb, B)
            assert info["qr_rank"] == int(ranks.sum()) and nmul == 1
            assert info["blockdiag_path"] == "batched-qr" and info["blockdiag_block"] == -1
            assert_blocks_close(x, ref, nb, 1e-8, 1e-10, ("undamped", nb, mb, B))
            assert np.array_equal(dy.get(), y)                # y is not clobbered


# ------------------------------------------------------------------------------------------ 2. rank-deficient blocks
@pytest.mark.parametrize("mb,nb,r", [(30, 12, 7), (9, 6, 5), (20, 8, 1), (6, 10, 4), (64, 33, 20), (300, 48, 1), (257, 64, 37)])
def test_rank_deficient_blocks_in_one_batch(ctx, mb, nb, r):
    """Eight blocks: deficient (randn(mb, r) @ randn(r, nb), seeded as in test_ldiv_qr) and full-rank ones alternating, one
    all-zero block (rank 0, x_b = 0).  Every block is compared."""
    rng = np.random.default_rng(100 + mb + nb + r)
    full = min(mb, nb)
    blocks, want = [], []
    for b in range(8):
        if b == 5:
            blocks.append(np.zeros((mb, nb))); want.append(0)
        elif b % 2 == 0:
            blocks.append(rng.standard_normal((mb, r)) @ rng.standard_normal((r, nb))); want.append(r)
        else:
            blocks.append(rng.standard_normal((mb, nb))); want.append(full)
    J = lsq.BlockDiagonal.from_blocks(blocks)
    y = rng.standard_normal(8 * mb)
    x, nmul, sv, _, _ = bq_solve(ctx, lsq.DeviceMatrix(ctx, J), y)
    ref, ranks = oracle_blocks(J, y)
    info = sv.info()
    print("ranks device", info["block_ranks"], "oracle", ranks, "intended", want)
    assert list(ranks) == want
    assert np.array_equal(info["block_ranks"], ranks) and info["qr_rank"] == sum(want) and nmul == 1
    assert_blocks_close(x, ref, nb, 1e-8, 1e-10, ("deficient", mb, nb, r))
    assert np.all(x[5 * nb:6 * nb] == 0.0)


# ------------------------------------------------------------------------------------------ 3. damped
@pytest.mark.parametrize("nb", NBS)
def test_damped_solve(ctx, nb):
    for mb in MBS:
        for B in (1, 7):
            J = make_bd(B, mb, nb, 3000 * nb + mb + B)
            rng = np.random.default_rng(nb * mb + B + 1)
            if B == 7 and mb == 40:
                J.block(3)[:, :] = 0.0                        # the batch with an all-zero block
            y = rng.standard_normal(B * mb)
            damp = 0.05 + rng.random(B * nb)
            Jd = lsq.DeviceMatrix(ctx, J)
            x, nmul, sv, dy, dd = bq_solve(ctx, Jd, y, damp)
            ref, ranks = oracle_blocks(J, y, damp)
            info = sv.info()
            assert np.all(ranks == nb) and np.array_equal(info["block_ranks"], ranks) and info["qr_rank"] == B * nb
            assert nmul == 1 and info["blockdiag_path"] == "batched-qr"
            assert_blocks_close(x, ref, nb, 1e-9, 1e-12, ("damped", nb, mb, B))
            assert np.array_equal(dd.get(), damp) and np.array_equal(dy.get(), y)      # neither is clobbered
            # the same handle column-scaled: J_b S_b
            s = 0.25 + rng.random(B * nb)
            Jd.set_colscale(lsq.DeviceVector(ctx, B * nb, s))
            JS = lsq.BlockDiagonal(B, mb, nb, data=J.data * np.repeat(s, mb))
            x, _, _, _, _ = bq_solve(ctx, Jd, y, damp)
            ref, _ = oracle_blocks(JS, y, damp)
            assert_blocks_close(x, ref, nb, 1e-9, 1e-12, ("damped scaled", nb, mb, B))
            x, _, sv, _, _ = bq_solve(ctx, Jd, y)
            ref, ranks = oracle_blocks(JS, y)
            assert np.array_equal(sv.info()["block_ranks"], ranks)
            assert_blocks_close(x, ref, nb, 1e-8, 1e-10, ("undamped scaled", nb, mb, B))
            Jd.set_colscale(None)


# ------------------------------------------------------------------------------------------ 4. ill-conditioned blocks
@pytest.mark.parametrize("cond", [1e6, 1e10])
@pytest.mark.parametrize("mb,nb", [(128, 32), (257, 64), (40, 17)])
def test_ill_conditioned_blocks(ctx, mb, nb, cond):
    """J_b = U diag(s) V', s = logspace(0, -log10(cond), nb), y = J x_true: a consistent system, so a backward-stable solve
    has |x - x_true| / |x_true| <= cond * 2.2e-16 to first order.  Measured on the CPU with the oracle and a numpy stand-in of
    the two-stage scheme: 2.6e-12 .. 1.6e-11 at cond 1e6, 1.5e-8 .. 7.6e-8 at cond 1e10.  The device must also stay within 16 x
    max(the oracle's own error on the same block, 1e-13): the factor covers the different reflector order."""
    B = 4
    rng = np.random.default_rng(int(np.log10(cond)) * 1000 + mb + nb)
    blocks, xt = [], rng.standard_normal(B * nb)
    for b in range(B):
        U, _ = np.linalg.qr(rng.standard_normal((mb, nb)))
        V, _ = np.linalg.qr(rng.standard_normal((nb, nb)))
        blocks.append(U @ np.diag(np.logspace(0, -np.log10(cond), nb)) @ V.T)
    J = lsq.BlockDiagonal.from_blocks(blocks)
    y = np.concatenate([blocks[b] @ xt[b * nb:(b + 1) * nb] for b in range(B)])
    x, _, sv, _, _ = bq_solve(ctx, lsq.DeviceMatrix(ctx, J), y)
    ref, ranks = oracle_blocks(J, y)
    assert np.all(ranks == nb) and np.array_equal(sv.info()["block_ranks"], ranks)
    for b in range(B):
        t = xt[b * nb:(b + 1) * nb]
        e_dev = np.linalg.norm(x[b * nb:(b + 1) * nb] - t) / np.linalg.norm(t)
        e_orc = np.linalg.norm(ref[b * nb:(b + 1) * nb] - t) / np.linalg.norm(t)
        print("cond %.0e %dx%d block %d: device %.3e oracle %.3e bound %.3e" % (cond, mb, nb, b, e_dev, e_orc, cond * 2.2e-16))
        assert e_dev <= cond * 2.2e-16, (b, e_dev)
        assert e_dev <= 16.0 * max(e_orc, 1e-13), (b, e_dev, e_orc)


# ------------------------------------------------------------------------------------------ 5. determinism
@pytest.mark.parametrize("nb", [8, 33])
def test_bits_do_not_depend_on_the_run_or_the_batch(ctx, nb):
    B, mb = 300, 40
    J = make_bd(B, mb, nb, 77 + nb)
    rng = np.random.default_rng(nb)
    y = rng.standard_normal(B * mb)
    damp = 0.05 + rng.random(B * nb)
    J1 = lsq.BlockDiagonal.from_blocks([J.block(5)])
    for d in (None, damp):
        Jd = lsq.DeviceMatrix(ctx, J)
        x1 = bq_solve(ctx, Jd, y, d)[0]
        x2 = bq_solve(ctx, Jd, y, d)[0]
        assert x1.tobytes() == x2.tobytes()
        xa = bq_solve(ctx, lsq.DeviceMatrix(ctx, J1), y[5 * mb:6 * mb], None if d is None else d[5 * nb:6 * nb])[0]
        assert xa.tobytes() == x1[5 * nb:6 * nb].tobytes()


# ------------------------------------------------------------------------------------------ 6. one trust region, stacked
@pytest.mark.parametrize("opt", ["lm", "dogleg"])
def test_one_trust_region_over_the_stacked_problem(ctx, opt):
    """optimize_ with LevenbergMarquardt(BlockQR()) / Dogleg(BlockQR()) on 6 full-rank blocks of 24 x 5 (the tanh model of
    test_c_gpu_blockdiag.py) against O.optimize(.., O.QR, ..) on the stacked dense Jacobian."""
    B, mb, nb = 6, 24, 5
    A, b, mv, (Jo, f, g, ud, keep) = tanh_setup(B, mb, nb, 7)
    Opt, ookind = (lsq.LevenbergMarquardt, O.LM) if opt == "lm" else (lsq.Dogleg, O.DOGLEG)
    ro = O.optimize(ookind, O.QR, Jo, np.zeros(B * nb), f, g, ud=ud, iterations=50)
    assert ro.status == 0 and ro.converged
    rh = lsq.optimize_(stacked_host_problem(A, b, mv), Opt(lsq.BlockQR()), full_trace=True, iterations=50, ctx=ctx)
    print(opt, "iterations", rh.iterations, ro.iterations, "ssr", rh.ssr, ro.ssr)
    assert rh.iterations == ro.iterations and rh.converged
    assert (rh.f_calls, rh.g_calls, rh.mul_calls) == (ro.f_calls, ro.g_calls, ro.mul_calls)
    assert (rh.x_converged, rh.f_converged, rh.g_converged) == (ro.x_converged, ro.f_converged, ro.g_converged)
    assert compare_until_roundoff(rh, ro, ssr0=float(np.sum(b * b))) is None
    assert np.max(np.abs(rh.minimizer - ro.minimizer)) <= 1e-8 * max(1.0, np.max(np.abs(ro.minimizer)))
    # ... and through the allocated problem
    nlsa = lsq.LeastSquaresProblemAllocated(stacked_host_problem(A, b, mv), Opt(lsq.BlockQR()), ctx=ctx)
    ra = lsq.optimize_(nlsa, iterations=50)
    assert ra.iterations == ro.iterations and np.array_equal(ra.minimizer, rh.minimizer)
    nlsa.free()


# ------------------------------------------------------------------------------------------ 7. one trust region per block
RB, RMB, RNB = 9, 24, 4
REDUNDANT = (2, 6)


def redundant_setup():
    """9 blocks of 24 x 4, r_b = A_b tanh(u_b) - b_b.  Blocks 2 and 6: u = (x0 + x1, x0 + x1, x2, x3) with EQUAL columns 0 and 1
    of A_b (sixteen 2.0 over eight 0.0), so J_b has two identical columns -- rank 3 -- at every x, and at x0 = 0 their Gram
    entries are 256 exactly: the pivoted Cholesky meets an exact zero pivot.  The other blocks: u = x, Gaussian A_b."""
    rng = np.random.default_rng(2024)
    A = rng.standard_normal((RB, RMB, RNB)) * 0.5
    col = np.concatenate([np.full(16, 2.0), np.zeros(8)])
    for k in REDUNDANT:
        A[k, :, 0] = col
        A[k, :, 1] = col
    xt = rng.uniform(-0.5, 0.5, (RB, RNB))
    b = np.stack([A[k] @ np.tanh(u_of(k, xt[k])) for k in range(RB)]) + 1e-3 * rng.standard_normal((RB, RMB))
    return A, b


def u_of(k, x):
    if k in REDUNDANT:
        return np.array([x[0] + x[1], x[0] + x[1], x[2], x[3]])
    return x


def block_f(A, b, k, x):
    return A[k] @ np.tanh(u_of(k, x)) - b[k]


def block_jac(A, k, x):
    """d r_b / d x: column j = A[:, j] (1 - tanh(u_j)^2) for a plain block; the redundant pair shares u_0 = u_1 = x0 + x1, so
    both of its columns are (A[:, 0] + A[:, 1]) (1 - tanh(x0 + x1)^2) = 2 A[:, 0] (1 - tanh(x0 + x1)^2)."""
    w = 1.0 - np.tanh(u_of(k, x)) ** 2
    Jb = A[k] * w
    if k in REDUNDANT:
        c = (A[k][:, 0] + A[k][:, 1]) * w[0]
        Jb[:, 0] = c
        Jb[:, 1] = c
    return Jb


def redundant_problem(A, b):
    def f_(out, x):
        for k in range(RB):
            out[k * RMB:(k + 1) * RMB] = block_f(A, b, k, x[k * RNB:(k + 1) * RNB])

    def g_(J, x):
        for k in range(RB):
            J.block(k)[:, :] = block_jac(A, k, x[k * RNB:(k + 1) * RNB])

    return lsq.LeastSquaresProblem(x=np.zeros(RB * RNB), y=np.zeros(RB * RMB), f_=f_, g_=g_, J=lsq.BlockDiagonal(RB, RMB, RNB))


def redundant_oracle(A, b, k, okind, lower=None, upper=None, iterations=50):
    def f(out, x):
        out[:] = block_f(A, b, k, x)

    def g(Jv, x):
        Jv[:] = block_jac(A, k, x).reshape(-1, order="F")

    kw = {} if lower is None else dict(lower=lower[k * RNB:(k + 1) * RNB], upper=upper[k * RNB:(k + 1) * RNB])
    return O.optimize(okind, O.QR, O.Mat(dense=np.zeros((RMB, RNB))), np.zeros(RNB), f, g, iterations=iterations, **kw)


def check_block(rb, ro, label):
    assert ro.status == 0 and rb.status == 0, (label, rb.status, ro.status)
    same_counts(rb, ro, label)
    ex = compare_until_roundoff(rb, ro, ssr0=rb.ssr0)
    print(label, "iterations", rb.iterations, "ssr %.12e / %.12e" % (rb.ssr, ro.ssr), "info", rb.info, "excused" if ex is not None else "")
    assert abs(rb.ssr - ro.ssr) <= 1e-9 * ro.ssr, label
    assert np.max(np.abs(rb.minimizer - ro.minimizer)) <= 1e-8 * max(1.0, np.max(np.abs(ro.minimizer))), label
    return ex is not None


@pytest.mark.parametrize("opt", ["lm", "dogleg"])
def test_batched_loop_with_redundant_blocks(ctx, opt):
    """Per block against the oracle's optimize(.., O.QR, ..) on that block alone.  What the operand does today: with
    Dogleg(Cholesky()) the two redundant blocks end with LSQ_ERANK.  With BlockQR() every block converges with status 0.
    info[b] is the rank of the block's last solve: 3 for the redundant blocks under Dogleg (the undamped J_b); under
    LevenbergMarquardt the matrix that is factored is [J_b; diag(sqrt(damp_b))], whose rank is nb for any positive damping --
    there the oracle's own damped solve says 4 too."""
    Opt, okind = (lsq.LevenbergMarquardt, O.LM) if opt == "lm" else (lsq.Dogleg, O.DOGLEG)
    A, b = redundant_setup()
    if opt == "dogleg":
        rc = lsq.optimize_batched_(redundant_problem(A, b), lsq.Dogleg(lsq.Cholesky()), iterations=50, ctx=ctx)
        assert all(rc.status[k] == lsq._lib.ERANK for k in REDUNDANT)
        assert all(rc.status[k] == 0 for k in range(RB) if k not in REDUNDANT)
    ros = [redundant_oracle(A, b, k, okind) for k in range(RB)]
    assert all(ro.status == 0 and ro.converged for ro in ros)
    r = lsq.optimize_batched_(redundant_problem(A, b), Opt(lsq.BlockQR()), iterations=50, full_trace=True, ctx=ctx)
    assert np.all(r.status == 0) and np.all(r.converged == 1)
    excused = sum(check_block(r.block(k), ros[k], (opt, k)) for k in range(RB))
    assert excused <= 1
    for k in range(RB):
        assert r.info[k] == (3 if (k in REDUNDANT and opt == "dogleg") else RNB), (k, r.info)
        assert np.array_equal(r.block(k).trace["inner"], ros[k].trace["inner"])
    # bounds on one block.  Dogleg converges there (26 iterations in the oracle); the reference's LM creeps along active
    # bounds and does not converge within 50 iterations for any box tried on the CPU (as in test_d_gpu_batched.py::
    # test_bounds), so LM is compared over 25 iterations
    nit = 50 if opt == "dogleg" else 25
    n = RB * RNB
    lower, upper = np.full(n, -np.inf), np.full(n, np.inf)
    lower[4 * RNB:5 * RNB], upper[4 * RNB:5 * RNB] = -0.1, 0.15
    ros[4] = redundant_oracle(A, b, 4, okind, lower=lower, upper=upper, iterations=nit)
    rbnd = lsq.optimize_batched_(redundant_problem(A, b), Opt(lsq.BlockQR()), iterations=nit, lower=lower, upper=upper,
                                 full_trace=True, ctx=ctx)
    assert np.all(rbnd.status == 0)
    x4 = rbnd.block(4).minimizer
    assert np.all(x4 >= -0.1) and np.all(x4 <= 0.15) and (np.any(x4 == -0.1) or np.any(x4 == 0.15))
    check_block(rbnd.block(4), ros[4], (opt, "bounded block"))
    assert opt == "lm" or rbnd.converged[4] == 1
    for k in (0, 2):
        check_block(rbnd.block(k), ros[k], (opt, "beside the bounded block", k))


# ------------------------------------------------------------------------------------------ 7b. workgroup-per-block geometry
def tanh_block_oracle(A, b, x0, k, okind):
    mb, nb = A.mb, A.nb
    Ab, bb = np.ascontiguousarray(A.block(k)), b[k * mb:(k + 1) * mb].copy()

    def f(out, x):
        out[:] = Ab @ np.tanh(x) - bb

    def g(Jv, x):
        Jv[:] = (Ab * (1.0 - np.tanh(x) ** 2)).reshape(-1, order="F")

    return O.optimize(okind, O.QR, O.Mat(dense=np.zeros((mb, nb))), x0[k * nb:(k + 1) * nb], f, g, iterations=50)


@pytest.mark.parametrize("opt", ["lm", "dogleg"])
@pytest.mark.parametrize("B,mb,nb", [(5, 40, 20), (6, 150, 33), (3, 100, 64)])
def test_batched_loop_one_workgroup_per_block(ctx, B, mb, nb, opt):
    """nb > 16: the batched loop's operands of the kernel (mask, r_b = J_b'f_b, diag(J_b'J_b), LM's damping formed in the
    kernel) in the one-workgroup-per-block geometry, with one, three and two chunks of rows.  Every block against the oracle's
    optimize(.., O.QR, ..) on that block alone; blocks start from different points (at 40 x 20 under LM and at 100 x 64 under
    Dogleg they then stop at different iterations, so blocks are masked out while others go on).  r_b directly: the first traced gradient norm is max|J_b(x0)'f_b(x0)|, formed here with numpy
    (a sum of mb products per entry: 1e-12 relative covers its rounding many times over).  diag(J_b'J_b) has no output of its
    own: it is LM's damping and Dogleg's scaling, so it is checked by the trajectories."""
    Opt, okind = (lsq.LevenbergMarquardt, O.LM) if opt == "lm" else (lsq.Dogleg, O.DOGLEG)
    A, b, x0 = plain_problem(B, mb, nb, 11 + nb)
    sign = np.where(np.arange(nb) % 2 == 0, 1.0, -1.0)
    for k in range(B):
        x0[k * nb:(k + 1) * nb] = 0.2 * (k % 3) * sign
    ros = [tanh_block_oracle(A, b, x0, k, okind) for k in range(B)]
    assert all(ro.status == 0 and ro.converged for ro in ros)
    r = lsq.optimize_batched_(batched_host_problem(A, b, x0), Opt(lsq.BlockQR()), iterations=50, full_trace=True, ctx=ctx)
    assert np.all(r.status == 0) and np.all(r.converged == 1) and np.all(r.info == nb)
    excused = sum(check_block(r.block(k), ros[k], (opt, B, mb, nb, k)) for k in range(B))
    assert excused <= 1
    for k in range(B):
        xk = x0[k * nb:(k + 1) * nb]
        Jk = A.block(k) * (1.0 - np.tanh(xk) ** 2)
        g0 = np.max(np.abs(Jk.T @ (A.block(k) @ np.tanh(xk) - b[k * mb:(k + 1) * mb])))
        assert abs(r.block(k).trace["gnorm"][0] - g0) <= 1e-12 * g0, (k, r.block(k).trace["gnorm"][0], g0)
    r2 = lsq.optimize_batched_(batched_host_problem(A, b, x0), Opt(lsq.BlockQR()), iterations=50, full_trace=True, ctx=ctx)
    assert r2.minimizer.tobytes() == r.minimizer.tobytes() and r2.trace["gnorm"].tobytes() == r.trace["gnorm"].tobytes()


# ------------------------------------------------------------------------------------------ 8. refusals
def test_refusals(ctx):
    J = make_bd(4, 16, 8, 1)
    Jd = lsq.DeviceMatrix(ctx, J)
    for other in (lsq.DeviceMatrix(ctx, J.toarray()), lsq.DeviceMatrix(ctx, J.tocsc())):
        with pytest.raises(lsq.ArgumentError) as e:
            lsq.AllocatedSolver(other, lsq.BlockQR(), for_lm=False)
        assert e.value.status == lsq._lib.EARG and "64 x 32" in str(e.value)
    J65 = lsq.DeviceMatrix(ctx, make_bd(2, 70, 65, 1))
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.AllocatedSolver(J65, lsq.BlockQR(), for_lm=True)
    assert e.value.status == lsq._lib.EARG and "70 x 65" in str(e.value)
    pr = lsq.synthetic.TanhProblem(140, 130, ctx=ctx, blockdiag=(2, 70, 65))
    with pytest.raises(lsq.ArgumentError) as e:
        pr.optimize_batched(lsq._lib.DOGLEG, lsq._lib.BLOCK_QR)
    assert e.value.status == lsq._lib.EARG and "70 x 65" in str(e.value)
    pr.close()
    # QR() stays refused on the very same handle, with its old text
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.AllocatedSolver(Jd, lsq.QR(), for_lm=False)
    assert str(e.value) == "solver QR() is not available for sparse Jacobians. Choose between Cholesky() and LSMR()"
    # a solver allocated for one block shape refuses another handle
    sv = lsq.AllocatedSolver(Jd, lsq.BlockQR(), for_lm=False)
    sv.J = lsq.DeviceMatrix(ctx, make_bd(2, 32, 16, 1))         # same m x n, other blocks
    with pytest.raises(lsq.DimensionMismatch) as e:
        sv.ldiv_(lsq.DeviceVector(ctx, 32), lsq.DeviceVector(ctx, 64))
    assert e.value.status == lsq._lib.EDIM
    # the per-block ranks belong to BlockQR()
    sc = lsq.AllocatedSolver(Jd, lsq.Cholesky(), for_lm=True)
    ranks = (C.c_int * 4)()
    assert lsq.lib().lsq_solver_blockdiag_ranks(sc.h, ranks) == lsq._lib.EARG
    assert sc.info()["block_ranks"] is None
