"""Parameter covariance on the device (lsq_solver_covariance: k_bd_cov on block-diagonal handles, k_bb_cov_schur /
k_bb_cov_back behind the bordered elimination) against numpy: inv(A'A) per block, and inv(J'J) of the dense toarray() for the
bordered handle, from which the diagonal blocks are cut.

Tolerance: the project's for one direct solve (tests/gpu_common.py: rel 1e-9), as ||Cov - ref||_F / ||ref||_F per block.  The
operands are the library's generator (N(0,1)/sqrt(mb)); the standard bound c nb eps cond(J_b'J_b) stays orders below it on
every shape here (the worst, one square 64 x 64 block, has cond ~ 5e4: numpy's own inverse differs from a QR-based one by
1e-12 there)."""
import ctypes as C

import numpy as np
import pytest

from gpu_common import lsq

pytestmark = pytest.mark.gpu

SOLVE_RTOL = 1e-9        # gpu_common: one direct solve
EARG = lsq._lib.EARG


def make_bd(B, mb, nb, seed):
    return lsq.BlockDiagonal(B, mb, nb, data=lsq.synthetic.blockdiag_inputs(B, mb, nb, seed))


def make_bb(B, mb, nb, ng, seed):
    return lsq.BorderedBlockDiagonal(B, mb, nb, ng, data=lsq.synthetic.bordered_inputs(B, mb, nb, ng, seed))


def rel_err(x, ref):
    return np.linalg.norm(x - ref) / np.linalg.norm(ref)


def block_refs(J):
    return [np.linalg.inv(J.block(b).T @ J.block(b)) for b in range(J.nblocks)]


def check_stderr(cov, B, nb, ng=0):
    """stderr is the square root of the diagonal of what was written to cov, in parameter order"""
    diag = np.concatenate([np.diag(cov.block(b)) for b in range(B)] + ([np.diag(cov.shared)] if ng else []))
    assert cov.stderr.shape == (B * nb + ng,)
    assert np.all(np.abs(cov.stderr - np.sqrt(diag)) <= 1e-15 * np.sqrt(diag))


def bd_cov(ctx, J, f=None):
    Jd = lsq.DeviceMatrix(ctx, J)
    sv = lsq.AllocatedSolver(Jd, lsq.Cholesky(), for_lm=True)
    return sv.covariance(f=f)


# ------------------------------------------------------------------------------------------ 1. block-diagonal, every branch
@pytest.mark.parametrize("nb", [1, 5, 16, 17, 32, 33, 48, 64])
@pytest.mark.parametrize("B,mb", [(7, 70), (1, 64)])
def test_blockdiag_every_branch(ctx, B, mb, nb):
    """One wavefront per block (nb <= 16; B = 7 leaves a half-empty workgroup of four) and one workgroup per block with 2, 3, 4
    tile rows, full and partial (33, 48); 70 rows = two full chunks and a partial one."""
    J = make_bd(B, mb, nb, 100 * nb + mb + B)
    refs = block_refs(J)
    for for_lm in (True, False):                           # either flavour of the Cholesky() solver is accepted
        sv = lsq.AllocatedSolver(lsq.DeviceMatrix(ctx, J), lsq.Cholesky(), for_lm=for_lm)
        cov = sv.covariance()
        assert np.array_equal(cov.info, np.zeros(B, dtype=np.int32))
        for b in range(B):
            err = rel_err(cov.block(b), refs[b])
            print("cov B=%d mb=%d nb=%d block %d rel err %.3e" % (B, mb, nb, b, err))
            assert err <= SOLVE_RTOL, (b, err)
            assert np.array_equal(cov.block(b), cov.block(b).T)
        check_stderr(cov, B, nb)
    f = np.random.default_rng(nb + mb).standard_normal(B * mb)
    if mb <= nb:                                           # no degrees of freedom left: refused
        with pytest.raises(lsq.ArgumentError):
            sv.covariance(f=f)
        return
    cov = sv.covariance(f=f)
    assert np.array_equal(cov.info, np.zeros(B, dtype=np.int32))
    for b in range(B):
        s2 = np.sum(f[b * mb:(b + 1) * mb] ** 2) / (mb - nb)
        err = rel_err(cov.block(b), s2 * refs[b])
        print("cov with f B=%d mb=%d nb=%d block %d rel err %.3e" % (B, mb, nb, b, err))
        assert err <= SOLVE_RTOL, (b, err)
        assert np.array_equal(cov.block(b), cov.block(b).T)
    check_stderr(cov, B, nb)
    # stderr alone (d_cov = NULL) is the same numbers
    Jd = sv.J
    dse = lsq.DeviceVector(ctx, Jd.n)
    lsq._lib.check(lsq.lib().lsq_solver_covariance(sv.h, Jd.h, lsq.DeviceVector(ctx, Jd.m, f).ptr, None, dse.ptr, None))
    assert np.array_equal(dse.get(), cov.stderr)


# ------------------------------------------------------------------------------------------ 2. column-scaled handle
@pytest.mark.parametrize("B,mb,nb", [(7, 70, 5), (7, 70, 40)])
def test_blockdiag_column_scaled(ctx, B, mb, nb):
    V = make_bd(B, mb, nb, 11)
    rng = np.random.default_rng(B + nb)
    s = 0.25 + rng.random(B * nb)
    f = rng.standard_normal(B * mb)
    Jd = lsq.DeviceMatrix(ctx, V)
    ds = lsq.DeviceVector(ctx, B * nb, s)
    Jd.set_colscale(ds)
    sv = lsq.AllocatedSolver(Jd, lsq.Cholesky(), for_lm=True)
    JS = lsq.BlockDiagonal(B, mb, nb, data=V.data * np.repeat(s, mb))
    for ff in (None, f):
        cov, mult = sv.covariance(f=ff), bd_cov(ctx, JS, f=ff)
        refs = block_refs(JS)
        for b in range(B):
            s2 = 1.0 if ff is None else np.sum(f[b * mb:(b + 1) * mb] ** 2) / (mb - nb)
            assert rel_err(cov.block(b), mult.block(b)) <= SOLVE_RTOL
            assert rel_err(cov.block(b), s2 * refs[b]) <= SOLVE_RTOL
        check_stderr(cov, B, nb)


# ------------------------------------------------------------------------------------------ 3. a failing block
@pytest.mark.parametrize("nb,k", [(5, 2), (20, 17)])
def test_blockdiag_failing_block(ctx, nb, k):
    """An all-zero column has an exactly zero Gram pivot (0 - 0 in any order): block 3 reports column k + 1 and is NaN, the
    call succeeds, and the other blocks carry the bits of the same call on the handle without the defect."""
    B, mb = 6, 70
    good = make_bd(B, mb, nb, 21)
    bad = make_bd(B, mb, nb, 21)
    bad.block(3)[:, k] = 0.0
    f = np.random.default_rng(nb).standard_normal(B * mb)
    for ff in (None, f):
        cg, cb = bd_cov(ctx, good, f=ff), bd_cov(ctx, bad, f=ff)
        assert list(cb.info) == [0, 0, 0, k + 1, 0, 0]
        assert np.all(np.isnan(cb.block(3))) and np.all(np.isnan(cb.stderr[3 * nb:4 * nb]))
        for b in (0, 1, 2, 4, 5):
            assert np.array_equal(cb.block(b), cg.block(b))
            assert np.array_equal(cb.stderr[b * nb:(b + 1) * nb], cg.stderr[b * nb:(b + 1) * nb])


# ------------------------------------------------------------------------------------------ 4. independence, repeatability
@pytest.mark.parametrize("nb", [8, 40])
def test_blockdiag_independence_and_repeatability(ctx, nb):
    B, mb = 300, 70
    J = make_bd(B, mb, nb, 31)
    f = np.random.default_rng(nb).standard_normal(B * mb)
    Jd = lsq.DeviceMatrix(ctx, J)
    sv = lsq.AllocatedSolver(Jd, lsq.Cholesky(), for_lm=True)
    runs = [sv.covariance(f=f) for _ in range(2)]
    assert np.array_equal(runs[0].cov, runs[1].cov) and np.array_equal(runs[0].stderr, runs[1].stderr)
    lsq.debug_set(serial=1)
    try:
        ser = sv.covariance(f=f)
    finally:
        lsq.debug_set(serial=0)
    assert np.array_equal(ser.cov, runs[0].cov) and np.array_equal(ser.stderr, runs[0].stderr)
    alone = bd_cov(ctx, lsq.BlockDiagonal(1, mb, nb, data=np.asfortranarray(J.block(2)).reshape(-1, order="F")),
                   f=f[2 * mb:3 * mb])
    assert np.array_equal(alone.block(0), runs[0].block(2))
    assert np.array_equal(alone.stderr, runs[0].stderr[2 * nb:3 * nb])
    assert rel_err(runs[0].block(2), np.sum(f[2 * mb:3 * mb] ** 2) / (mb - nb) * block_refs(J)[2]) <= SOLVE_RTOL


# ------------------------------------------------------------------------------------------ 5. bordered
def check_bordered(cov, ref, B, nb, ng, s2, label):
    for b in range(B):
        r = s2 * ref[b * nb:(b + 1) * nb, b * nb:(b + 1) * nb]
        err = rel_err(cov.block(b), r)
        assert err <= SOLVE_RTOL, (label, b, err)
        assert np.array_equal(cov.block(b), cov.block(b).T)
    err = rel_err(cov.shared, s2 * ref[B * nb:, B * nb:])
    print(label, "shared block rel err %.3e" % err)
    assert err <= SOLVE_RTOL, (label, err)
    assert np.array_equal(cov.shared, cov.shared.T)
    assert cov.info is None
    check_stderr(cov, B, nb, ng)


@pytest.mark.parametrize("nb,ng", [(1, 1), (3, 2), (8, 8), (15, 1), (16, 1), (20, 12), (32, 16), (1, 63), (63, 1), (40, 24)])
def test_bordered_every_shape(ctx, nb, ng):
    """One wavefront per block (nb + ng <= 16) and one workgroup per block with 2, 3, 4 tile rows, the shared part the smallest
    and the largest share; one block, a grid that ends inside a workgroup of four, and 70 blocks (k_bb_reduce)."""
    mb = 96
    for B in (1, 5, 70):
        J = make_bb(B, mb, nb, ng, 1000 * nb + 10 * ng + B)
        D = J.toarray()
        ref = np.linalg.inv(D.T @ D)
        m, n = D.shape
        sv = lsq.AllocatedSolver(lsq.DeviceMatrix(ctx, J), lsq.Cholesky(), for_lm=True)
        check_bordered(sv.covariance(), ref, B, nb, ng, 1.0, (nb, ng, B))
        f = np.random.default_rng(nb + ng + B).standard_normal(m)
        check_bordered(sv.covariance(f=f), ref, B, nb, ng, np.sum(f ** 2) / (m - n), (nb, ng, B, "f"))
        assert sv.info()["blockdiag_path"] == "bordered-schur" and sv.info()["blockdiag_block"] == -1


def test_bordered_repeatability_and_serial_mode(ctx):
    B, mb, nb, ng = 70, 96, 20, 12
    J = make_bb(B, mb, nb, ng, 5)
    f = np.random.default_rng(1).standard_normal(B * mb)
    sv = lsq.AllocatedSolver(lsq.DeviceMatrix(ctx, J), lsq.Cholesky(), for_lm=True)
    runs = [sv.covariance(f=f) for _ in range(2)]
    assert np.array_equal(runs[0].cov, runs[1].cov) and np.array_equal(runs[0].stderr, runs[1].stderr)
    lsq.debug_set(serial=1)
    try:
        ser = sv.covariance(f=f)
    finally:
        lsq.debug_set(serial=0)
    assert np.array_equal(ser.cov, runs[0].cov) and np.array_equal(ser.stderr, runs[0].stderr)


# ------------------------------------------------------------------------------------------ 6. bordered failure
@pytest.mark.parametrize("nb,ng", [(20, 6), (5, 3)])
def test_bordered_not_positive_definite(ctx, nb, ng):
    """A zero local column: LSQ_ENOTPD with the stacked column and block that lsq_ldiv_damped with zero damping reports for the
    same handle."""
    B, mb, kl = 5, 96, 3
    J = make_bb(B, mb, nb, ng, 7)
    J.block(2)[:, kl] = 0.0
    n, m = B * nb + ng, B * mb
    Jd = lsq.DeviceMatrix(ctx, J)
    sv = lsq.AllocatedSolver(Jd, lsq.Cholesky(), for_lm=True)
    with pytest.raises(lsq.PosDefException) as es:
        sv.ldiv_(lsq.DeviceVector(ctx, n), lsq.DeviceVector(ctx, m, np.ones(m)), lsq.DeviceVector(ctx, n))
    solve_info = sv.info()
    sv2 = lsq.AllocatedSolver(Jd, lsq.Cholesky(), for_lm=True)
    with pytest.raises(lsq.PosDefException) as ec:
        sv2.covariance()
    assert ec.value.status == lsq._lib.ENOTPD
    assert str(ec.value) == str(es.value) == "PosDefException: matrix is not positive definite; Cholesky failed at %d" % (2 * nb + kl + 1)
    info = sv2.info()
    assert (info["blockdiag_path"], info["blockdiag_block"]) == (solve_info["blockdiag_path"], solve_info["blockdiag_block"])
    assert info["blockdiag_block"] == 2
    h_info = np.full(1, -5, dtype=np.int32)
    dcov = lsq.DeviceVector(ctx, B * nb * nb + ng * ng)
    rc = lsq.lib().lsq_solver_covariance(sv2.h, Jd.h, None, dcov.ptr, None, h_info.ctypes.data_as(lsq._lib.c_ip))
    assert rc == lsq._lib.ENOTPD and h_info[0] == 2 * nb + kl + 1


# ------------------------------------------------------------------------------------------ 7. refusals through the C ABI
def test_refusals(ctx):
    L = lsq.lib()
    B, mb, nb = 4, 10, 3
    Jd = lsq.DeviceMatrix(ctx, make_bd(B, mb, nb, 1))
    out = lsq.DeviceVector(ctx, B * 64 * 64)
    f = lsq.DeviceVector(ctx, 64 * B)
    chol = lsq.AllocatedSolver(Jd, lsq.Cholesky(), for_lm=True)
    dense = lsq.DeviceMatrix(ctx, np.eye(6, 3))
    other = lsq.DeviceMatrix(ctx, make_bd(B, mb, 2, 1))
    square = lsq.DeviceMatrix(ctx, make_bd(B, nb, nb, 1))
    bb = lsq.DeviceMatrix(ctx, make_bb(B, mb, nb, 2, 1))
    wide_bb = lsq.DeviceMatrix(ctx, make_bb(1, 4, 3, 2, 1))                # m = 4 <= n = 5
    cases = [
        ("an LSMR solver", lsq.AllocatedSolver(Jd, lsq.LSMR(), for_lm=True), Jd, None, out.ptr, None),
        ("a BlockQR solver", lsq.AllocatedSolver(Jd, lsq.BlockQR(), for_lm=True), Jd, None, out.ptr, None),
        ("a dense handle", lsq.AllocatedSolver(dense, lsq.Cholesky(), for_lm=True), dense, None, out.ptr, None),
        ("another shape", chol, other, None, out.ptr, None),
        ("a bordered handle on a block-diagonal solver", chol, bb, None, out.ptr, None),
        ("a block-diagonal handle on a bordered solver", lsq.AllocatedSolver(bb, lsq.Cholesky(), for_lm=True), Jd, None, out.ptr, None),
        ("both outputs NULL", chol, Jd, None, None, None),
        ("mb <= nb with f", lsq.AllocatedSolver(square, lsq.Cholesky(), for_lm=True), square, f.ptr, out.ptr, None),
        ("m <= n with f, bordered", lsq.AllocatedSolver(wide_bb, lsq.Cholesky(), for_lm=True), wide_bb, f.ptr, out.ptr, None),
    ]
    for label, sv, J, pf, pcov, pse in cases:
        rc = L.lsq_solver_covariance(sv.h, J.h, pf, pcov, pse, None)
        msg = L.lsq_last_error().decode()
        print(label, "->", rc, msg)
        assert rc == EARG, (label, rc)
        assert msg.startswith("lsq_solver_covariance:"), (label, msg)
    with pytest.raises(lsq.ArgumentError):                                 # ... and as the Python exception
        lsq.covariance(dense)
    # the solver still works after the refusals
    assert np.array_equal(chol.covariance().info, np.zeros(B, dtype=np.int32))


# ------------------------------------------------------------------------------------------ 8. after a fit
def test_standard_errors_after_a_batched_fit(ctx):
    """B exponential decays a exp(-k t) + noise fitted at once (optimize_batched_), then the standard errors of (a_b, k_b) at
    the solution against numpy on the final Jacobian: sqrt(diag(ssr_b / (mb - 2) inv(J_b'J_b)))."""
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
    r = lsq.optimize_batched_(nls, lsq.LevenbergMarquardt(lsq.Cholesky()), iterations=100, ctx=ctx)
    assert all(r.block(b).converged for b in range(B))
    x = r.minimizer
    Jf = lsq.BlockDiagonal(B, mb, nb, data=jac(x).reshape(-1))
    fres = (model(x) - data).reshape(-1)
    cov = lsq.covariance(lsq.DeviceMatrix(ctx, Jf), f=fres)
    assert np.array_equal(cov.info, np.zeros(B, dtype=np.int32))
    for b in range(B):
        A = Jf.block(b)
        ref = np.sqrt(np.diag(np.sum(fres[b * mb:(b + 1) * mb] ** 2) / (mb - nb) * np.linalg.inv(A.T @ A)))
        got = cov.stderr[b * nb:(b + 1) * nb]
        print("fit block %d stderr %s ref %s" % (b, got, ref))
        assert np.all(np.abs(got - ref) <= SOLVE_RTOL * ref)
        assert np.all(got < 0.1)                                           # the parameters ARE determined (noise 1%)
