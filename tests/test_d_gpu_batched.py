"""optimize_batched_ / lsq_optimize_batched (lsq_batched.hip): B fits on a block-diagonal Jacobian with one trust region per
block, against the oracle run on EVERY BLOCK ALONE as a dense mb x nb problem (O.optimize(.., CHOLESKY, O.Mat(dense=..)) with
the tanh model restricted to the block).

Tolerances are the project's (tests/gpu_common.py, test_c_gpu_blockdiag.py): minimizers 1e-8, ssr 1e-9 relative, trajectories
through compare_until_roundoff with its defaults; counts, flags and statuses are compared exactly.

The heterogeneous trajectory problem: tanh_setup(16, 128, 32, 7) of test_c_gpu_blockdiag.py with block b started from
x0_b = HET_C * (b mod 4) * (+1, -1, +1, ...) and HET_NOISE * N(0,1) (generator stream seed + 303) added to the right-hand side
of the blocks with b mod 8 == 5.  The per-block oracle, run on the CPU before the inputs were fixed, converges on every block
within 50 iterations with LM iteration counts [6 6 6 11 6 7 6 11 6 6 6 11 6 5 6 11] and Dogleg counts
[6 6 11 13 6 7 6 16 6 6 6 6 6 6 6 7]; under O.set_sum_mode(6) (tree sums) against index-order sums the oracle itself changes
no LM accept decision and one Dogleg block's.  (HET_C = 0.6 with noise 0.5 leaves an LM block unconverged after 50 iterations
and, like noise >= 0.2 at HET_C = 0.3, drives some Dogleg blocks into saturated tanh and a rank-deficient factorisation.)"""
import numpy as np
import pytest

from gpu_common import compare_until_roundoff, lsq
from oracle import oracle as O

pytestmark = pytest.mark.gpu

TRAJ = (16, 128, 32)
TRAJ_SEED = 7
HET_C, HET_NOISE = 0.3, 0.1
OPT = {"lm": (lsq.LevenbergMarquardt, lsq._lib.LEVENBERG_MARQUARDT, O.LM), "dogleg": (lsq.Dogleg, lsq._lib.DOGLEG, O.DOGLEG)}


def make_A(B, mb, nb, seed):
    return lsq.BlockDiagonal(B, mb, nb, data=lsq.synthetic.blockdiag_inputs(B, mb, nb, seed))


def block_mv(A, t):
    """A t block by block (one dgemv per block: a block's rows do not depend on which other blocks are in the batch)."""
    out = np.empty(A.shape[0])
    for k in range(A.nblocks):
        out[k * A.mb:(k + 1) * A.mb] = A.block(k) @ t[k * A.nb:(k + 1) * A.nb]
    return out


def plain_problem(B, mb, nb, seed):
    A = make_A(B, mb, nb, seed)
    _, b = lsq.synthetic.rhs_for(lambda t: block_mv(A, t), B * mb, B * nb, seed)
    return A, b, np.zeros(B * nb)


def het_problem():
    B, mb, nb = TRAJ
    A, b, x0 = plain_problem(B, mb, nb, TRAJ_SEED)
    noise = lsq.synthetic.normal(B * mb, TRAJ_SEED + 303)
    sign = np.where(np.arange(nb) % 2 == 0, 1.0, -1.0)
    for k in range(B):
        x0[k * nb:(k + 1) * nb] = HET_C * (k % 4) * sign
        if k % 8 == 5:
            b[k * mb:(k + 1) * mb] += HET_NOISE * noise[k * mb:(k + 1) * mb]
    return A, b, x0


def host_problem(A, b, x0, poison=None):
    """Host-side f_ / g_ on the stacked vectors, block-separable and deterministic.  poison(k, calls) -> True makes block k's
    rows of f_ NaN at that call."""
    B, mb, nb = A.nblocks, A.mb, A.nb
    calls = [0]

    def f_(out, x):
        calls[0] += 1
        out[:] = block_mv(A, np.tanh(x)) - b
        if poison is not None:
            for k in range(B):
                if poison(k, calls[0]):
                    out[k * mb:(k + 1) * mb] = np.nan

    def g_(J, x):
        J.data[:] = A.data * np.repeat(1.0 - np.tanh(x) ** 2, mb)

    return lsq.LeastSquaresProblem(x=x0.copy(), y=np.zeros(B * mb), f_=f_, g_=g_, J=lsq.BlockDiagonal(B, mb, nb))


def block_oracle(A, b, x0, k, okind, iterations=50, lower=None, upper=None, nan_from_call=None):
    """The reference for block k: the oracle on that block alone as a dense mb x nb problem."""
    mb, nb = A.mb, A.nb
    Ab = np.ascontiguousarray(A.block(k))
    bb = b[k * mb:(k + 1) * mb].copy()
    calls = [0]

    def f(out, x):
        calls[0] += 1
        out[:] = Ab @ np.tanh(x) - bb
        if nan_from_call is not None and calls[0] >= nan_from_call:
            out[:] = np.nan

    def g(Jv, x):
        Jv[:] = (Ab * (1.0 - np.tanh(x) ** 2)).reshape(-1, order="F")

    kw = {}
    if lower is not None:
        kw = dict(lower=lower[k * nb:(k + 1) * nb], upper=upper[k * nb:(k + 1) * nb])
    return O.optimize(okind, O.CHOLESKY, O.Mat(dense=np.zeros((mb, nb))), x0[k * nb:(k + 1) * nb], f, g, iterations=iterations, **kw)


def device_run(ctx, A, b, x0, kind, **kw):
    B, mb, nb = A.nblocks, A.mb, A.nb
    pr = lsq.synthetic.TanhProblem(B * mb, B * nb, ctx=ctx, blockdiag=(B, mb, nb), inputs=A.data.copy(), b=b)
    pr.reset(x0)
    r = pr.optimize_batched(kind, lsq._lib.CHOLESKY, **kw)
    pr.close()
    return r


def same_counts(rb, ro, label):
    assert rb.iterations == ro.iterations, (label, rb.iterations, ro.iterations)
    assert (rb.f_calls, rb.g_calls, rb.mul_calls) == (ro.f_calls, ro.g_calls, ro.mul_calls), \
        (label, (rb.f_calls, rb.g_calls, rb.mul_calls), (ro.f_calls, ro.g_calls, ro.mul_calls))
    assert (rb.converged, rb.x_converged, rb.f_converged, rb.g_converged) == \
           (ro.converged, ro.x_converged, ro.f_converged, ro.g_converged), label


def same_as_oracle(r, ros, label, blocks=None, max_excused=1):
    """Every block of the batched result against its own oracle run: counts, flags, trace, minimizer."""
    excused = 0
    for k in (range(r.nblocks) if blocks is None else blocks):
        rb, ro = r.block(k), ros[k]
        assert ro.status == 0 and rb.status == 0, (label, k, rb.status, ro.status)
        same_counts(rb, ro, (label, k))
        ex = compare_until_roundoff(rb, ro, ssr0=rb.ssr0)
        print(label, "block", k, "iterations", rb.iterations, "ssr %.12e / %.12e" % (rb.ssr, ro.ssr),
              "max|dx| %.2e" % np.max(np.abs(rb.minimizer - ro.minimizer)), "excused" if ex is not None else "")
        excused += ex is not None
        assert abs(rb.ssr - ro.ssr) <= 1e-9 * ro.ssr, (label, k)
        assert np.max(np.abs(rb.minimizer - ro.minimizer)) <= 1e-8 * max(1.0, np.max(np.abs(ro.minimizer))), (label, k)
    assert excused <= max_excused, (label, excused)


# ------------------------------------------------------------------------------------------ 1. equals B separate oracle runs
@pytest.mark.parametrize("opt", ["lm", "dogleg"])
def test_equals_separate_oracle_runs(ctx, opt):
    Opt, kind, okind = OPT[opt]
    A, b, x0 = het_problem()
    B = A.nblocks
    ros = [block_oracle(A, b, x0, k, okind) for k in range(B)]
    its = [ro.iterations for ro in ros]
    print(opt, "oracle iterations per block", its)
    assert all(ro.status == 0 and ro.converged for ro in ros)
    assert len(set(its)) > 1                      # blocks really differ: a lock-step loop cannot pass
    rd = device_run(ctx, A, b, x0, kind, iterations=50, trace=True)
    assert rd.outer_iterations == max(its)
    same_as_oracle(rd, ros, opt + " device model")
    nls = host_problem(A, b, x0)
    rh = lsq.optimize_batched_(nls, Opt(lsq.Cholesky()), iterations=50, full_trace=True, ctx=ctx)
    assert rh.outer_iterations == max(its)
    same_as_oracle(rh, ros, opt + " host f_/g_")
    assert np.array_equal(rh.minimizer, nls.x)
    if opt == "lm":                               # the default optimizer here is LevenbergMarquardt(Cholesky())
        rdef = lsq.optimize_batched_(host_problem(A, b, x0), iterations=50, ctx=ctx)
        assert rdef.optimizer == "LevenbergMarquardt" and np.array_equal(rdef.iterations, rh.iterations)
        assert np.array_equal(rdef.minimizer, rh.minimizer)


# ------------------------------------------------------------------------------------------ 2. independence
def _bits(r, k):
    rb = r.block(k)
    return (rb.iterations, rb.ssr, rb.f_calls, rb.g_calls, rb.mul_calls, rb.minimizer.tobytes(), rb.trace["x"].tobytes(),
            rb.trace["ssr"].tobytes(), rb.trace["delta"].tobytes())


def sub_problem(A, b, x0, order):
    """The batch made of the blocks `order` (in that order)."""
    mb, nb = A.mb, A.nb
    A2 = lsq.BlockDiagonal.from_blocks([A.block(k) for k in order])
    b2 = np.concatenate([b[k * mb:(k + 1) * mb] for k in order])
    x2 = np.concatenate([x0[k * nb:(k + 1) * nb] for k in order])
    return A2, b2, x2


@pytest.mark.parametrize("opt", ["lm", "dogleg"])
def test_independence(ctx, opt):
    """The result for fit b is bit-identical in the batch of 16, alone in a batch of 1, and in the batch with the blocks
    permuted; across two runs; and under debug_set(serial=1).  f_ / g_ are the host callbacks (one dgemv per block, so the
    callbacks themselves give a block the same bits in every batch: the property under test is the loop's)."""
    Opt, kind, okind = OPT[opt]
    A, b, x0 = het_problem()
    B = A.nblocks
    run = lambda AA, bb, xx: lsq.optimize_batched_(host_problem(AA, bb, xx), Opt(lsq.Cholesky()), iterations=50, full_trace=True, ctx=ctx)
    r16 = run(A, b, x0)
    ref = [_bits(r16, k) for k in range(B)]
    again = run(A, b, x0)
    assert [_bits(again, k) for k in range(B)] == ref
    for k in (0, 3, 5, 7, 15):
        r1 = run(*sub_problem(A, b, x0, [k]))
        assert _bits(r1, 0) == ref[k], k
    perm = list(np.random.default_rng(3).permutation(B))
    rp = run(*sub_problem(A, b, x0, perm))
    for pos, k in enumerate(perm):
        assert _bits(rp, pos) == ref[k], (pos, k)
    lsq.debug_set(serial=1)
    try:
        rs = run(A, b, x0)
        rds = device_run(ctx, A, b, x0, kind, iterations=50, trace=True)
    finally:
        lsq.debug_set(serial=0)
    assert [_bits(rs, k) for k in range(B)] == ref
    # the device model: run to run and serialised
    rd = device_run(ctx, A, b, x0, kind, iterations=50, trace=True)
    rd2 = device_run(ctx, A, b, x0, kind, iterations=50, trace=True)
    assert [_bits(rd, k) for k in range(B)] == [_bits(rd2, k) for k in range(B)] == [_bits(rds, k) for k in range(B)]


# ------------------------------------------------------------------------------------------ 3. differs from the stacked loop
def test_differs_from_the_stacked_loop_where_it_should(ctx):
    """One trust region for the stack (optimize_, unchanged) and one per block both converge; the stacked run's iteration
    count is the stacked oracle's (dense 2048 x 512 Jacobian), the batched run's outer count is the maximum of the per-block
    oracle counts, and every block stops where ITS oracle run stops."""
    A, b, x0 = het_problem()
    B, mb, nb = TRAJ
    Ad = O.Mat(dense=A.toarray())
    f, g, ud, keep = O.tanh_model(Ad, b)
    rso = O.optimize(O.LM, O.CHOLESKY, O.Mat(dense=np.zeros(A.shape)), x0, f, g, ud=ud, iterations=50)
    assert rso.status == 0 and rso.converged
    rs = lsq.optimize_(host_problem(A, b, x0), lsq.LevenbergMarquardt(lsq.Cholesky()), iterations=50, full_trace=True, ctx=ctx)
    assert rs.converged and rs.iterations == rso.iterations
    assert (rs.f_calls, rs.g_calls, rs.mul_calls) == (rso.f_calls, rso.g_calls, rso.mul_calls)
    compare_until_roundoff(rs, rso, ssr0=float(np.sum((block_mv(A, np.tanh(x0)) - b) ** 2)))
    ros = [block_oracle(A, b, x0, k, O.LM) for k in range(B)]
    rb = lsq.optimize_batched_(host_problem(A, b, x0), lsq.LevenbergMarquardt(lsq.Cholesky()), iterations=50, ctx=ctx)
    assert np.all(rb.converged == 1)
    assert np.array_equal(rb.iterations, [ro.iterations for ro in ros])
    assert rb.outer_iterations == int(np.max(rb.iterations)) == max(ro.iterations for ro in ros)
    print("stacked iterations", rs.iterations, "| per-block", rb.iterations.tolist())
    assert abs(float(np.sum(rb.ssr)) - rs.ssr) <= 1e-6 * rs.ssr       # (both are at the same minimum of the separable objective)


# ------------------------------------------------------------------------------------------ 4. a failing block
def test_rank_deficient_block_under_dogleg(ctx):
    """The rank-deficient block of test_c_gpu_blockdiag.py::test_undamped_solve_and_rank_deficiency (64 ones over 64 zeros in
    columns 4 and 20 of block 11; x0 = 0, so J_11(x0) = A_11 has the exact duplicate): that block ends with
    RankDeficientException in its first iteration, like its own oracle run, holding x0; the other 15 equal their oracle runs."""
    B, mb, nb = TRAJ
    bad = 11
    A, b, x0 = plain_problem(B, mb, nb, TRAJ_SEED)
    col = np.zeros(mb)
    col[:64] = 1.0
    A.block(bad)[:, 4] = col
    A.block(bad)[:, 20] = col
    ros = [block_oracle(A, b, x0, k, O.DOGLEG) for k in range(B)]
    assert ros[bad].status == O.ERANK and all(ro.status == 0 and ro.converged for k, ro in enumerate(ros) if k != bad)
    others = [k for k in range(B) if k != bad]
    for label, r in (("device", device_run(ctx, A, b, x0, lsq._lib.DOGLEG, iterations=50, trace=True)),
                     ("host", lsq.optimize_batched_(host_problem(A, b, x0), lsq.Dogleg(lsq.Cholesky()), iterations=50,
                                                    full_trace=True, ctx=ctx))):
        rb, ro = r.block(bad), ros[bad]
        assert rb.status == lsq._lib.ERANK == ro.status and rb.info == nb - 1          # the block's own rank
        assert (rb.iterations, rb.f_calls, rb.g_calls, rb.mul_calls) == (ro.iterations, ro.f_calls, ro.g_calls, ro.mul_calls)
        assert not rb.converged
        assert np.array_equal(rb.minimizer, x0[bad * nb:(bad + 1) * nb]) and np.array_equal(rb.minimizer, ro.minimizer)
        same_as_oracle(r, ros, "rank-deficient " + label, blocks=others)
        assert r.status[bad] == lsq._lib.ERANK and np.all(r.status[others] == 0)


def test_nonfinite_residual_block_under_lm(ctx):
    """Block 6's rows of f_ are NaN from the second call on: every trial step of that block is refused (rho is NaN), its
    delta shrinks until the step meets x_tol -- exactly what its own oracle run does; the others are not disturbed."""
    B, mb, nb = TRAJ
    bad = 6
    A, b, x0 = het_problem()
    ros = [block_oracle(A, b, x0, k, O.LM, nan_from_call=2 if k == bad else None) for k in range(B)]
    r = lsq.optimize_batched_(host_problem(A, b, x0, poison=lambda k, c: k == bad and c >= 2), lsq.LevenbergMarquardt(lsq.Cholesky()),
                              iterations=50, full_trace=True, ctx=ctx)
    rb, ro = r.block(bad), ros[bad]
    print("NaN block: status", rb.status, ro.status, "iterations", rb.iterations, ro.iterations)
    assert rb.status == ro.status and rb.info == ro.bad_index
    same_counts(rb, ro, "nan block")
    assert np.array_equal(rb.trace["accept"], ro.trace["accept"]) and not np.any(rb.trace["accept"])
    assert np.max(np.abs(rb.minimizer - ro.minimizer)) <= 1e-8 and np.max(np.abs(rb.minimizer - x0[bad * nb:(bad + 1) * nb])) <= 1e-8
    assert rb.ssr == rb.ssr0                                           # the residual it held
    same_as_oracle(r, ros, "nan neighbours", blocks=[k for k in range(B) if k != bad])


def test_nonfinite_start_of_one_block(ctx):
    """check_isfinite per block: a block whose x0 holds an Inf is reported (LSQ_ENONFINITE, block-local index) with zero
    iterations, like its oracle run, and the rest of the batch runs."""
    B, mb, nb = TRAJ
    A, b, x0 = het_problem()
    x0[9 * nb + 13] = np.inf
    ro = block_oracle(A, b, x0, 9, O.LM)
    r = lsq.optimize_batched_(host_problem(A, b, x0), iterations=50, ctx=ctx)
    rb = r.block(9)
    assert ro.status == O.ENONFINITE and rb.status == lsq._lib.ENONFINITE and rb.info == ro.bad_index == 13
    assert (rb.iterations, rb.f_calls, rb.g_calls, rb.mul_calls) == (ro.iterations, ro.f_calls, ro.g_calls, ro.mul_calls) == (0, 1, 0, 0)
    assert np.all(r.converged[[k for k in range(B) if k != 9]] == 1)


# ------------------------------------------------------------------------------------------ 5. frozen means frozen
@pytest.mark.parametrize("opt", ["lm", "dogleg"])
def test_frozen_means_frozen(ctx, opt):
    """A host f_ that writes NaN into the rows of every FROZEN block.  x_b unchanged between two calls does not by itself
    mean frozen: under Dogleg a block whose Gauss-Newton step lies inside its trust region and is refused gets the SAME
    trial point again after delta has been halved (dogleg.jl:120-123, 193-194; blocks 2 and 3 here do), and poisoning that
    call would change the block's rho and with it its path.  So a block counts as frozen from the call after the last
    iteration of its own oracle run (call c is the trial point of outer iteration c - 1), and there f_ CHECKS that its
    entries of the trial point have not changed since the previous call -- they are the block's final x_b -- before it writes
    NaN.  Frozen blocks ignore it: the result equals the unpoisoned run bit for bit, and minimizer_b is the block's last
    accepted trace row."""
    Opt, kind, okind = OPT[opt]
    A, b, x0 = het_problem()
    B, mb, nb = TRAJ
    its = [block_oracle(A, b, x0, k, okind).iterations for k in range(B)]
    clean = lsq.optimize_batched_(host_problem(A, b, x0), Opt(lsq.Cholesky()), iterations=50, full_trace=True, ctx=ctx)
    prev, npoisoned, calls, moved = [None], [0], [0], []

    def f_(out, x):
        calls[0] += 1
        out[:] = block_mv(A, np.tanh(x)) - b
        for k in range(B):
            if calls[0] - 1 > its[k] + 1:       # (one call of slack: the first frozen call may follow a refused last step)
                if not np.array_equal(x[k * nb:(k + 1) * nb], prev[0][k * nb:(k + 1) * nb]):
                    moved.append((k, calls[0]))
                out[k * mb:(k + 1) * mb] = np.nan
                npoisoned[0] += 1
        prev[0] = x.copy()

    nls = host_problem(A, b, x0)
    nls.f_ = f_
    r = lsq.optimize_batched_(nls, Opt(lsq.Cholesky()), iterations=50, full_trace=True, ctx=ctx)
    assert npoisoned[0] > 0 and not moved, moved
    assert np.array_equal(r.iterations, its)
    assert np.array_equal(r.iterations, clean.iterations) and np.array_equal(r.minimizer, clean.minimizer)
    assert np.array_equal(r.ssr, clean.ssr) and np.all(np.isfinite(r.ssr)) and np.all(r.converged == 1)
    assert np.all(np.isfinite(nls.y))                                   # fcur of a frozen block is the residual it stopped with
    for k in range(B):
        rb = r.block(k)
        assert len(rb.trace["ssr"]) == rb.iterations                    # rows >= iterations[b] are never looked at
        if rb.trace["accept"][-1]:
            assert np.array_equal(rb.minimizer, rb.trace["x"][-1]) and rb.ssr == rb.trace["ssr"][-1]
        for key in ("f_calls", "g_calls", "mul_calls"):
            assert getattr(rb, key) == getattr(clean.block(k), key)


# ------------------------------------------------------------------------------------------ 6. shapes
@pytest.mark.parametrize("B,mb,nb,opts", [(300, 64, 8, ("lm", "dogleg")), (7, 3, 5, ("lm",)), (33, 257, 64, ("lm", "dogleg")),
                                          (1, 64, 16, ("lm", "dogleg"))])
def test_shapes(ctx, B, mb, nb, opts):
    """One wavefront per block with a grid that ends inside a workgroup of four (300 x 64 x 8), mb < nb (LM only: the undamped
    normal matrix is singular), four tile rows with a ragged last chunk (33 x 257 x 64), a single block."""
    A, b, x0 = plain_problem(B, mb, nb, 100 + B)
    for opt in opts:
        Opt, kind, okind = OPT[opt]
        ros = [block_oracle(A, b, x0, k, okind, iterations=100) for k in range(B)]
        assert all(ro.status == 0 and ro.converged for ro in ros)
        r = device_run(ctx, A, b, x0, kind, iterations=100)
        worst = 0.0
        for k in range(B):
            rb, ro = r.block(k), ros[k]
            assert rb.status == 0 and rb.converged, (opt, k)
            worst = max(worst, np.max(np.abs(rb.minimizer - ro.minimizer)) / max(1.0, np.max(np.abs(ro.minimizer))))
        print("shape", (B, mb, nb), opt, "outer", r.outer_iterations, "worst minimizer error %.3e" % worst)
        assert worst <= 1e-8
        assert r.outer_iterations == int(np.max(r.iterations))


# ------------------------------------------------------------------------------------------ 7. bounds
@pytest.mark.parametrize("opt", ["lm", "dogleg"])
def test_bounds(ctx, opt):
    """test_c_gpu_blockdiag.py::test_bounds' box [-0.7, 0.8] and 25 iterations, block by block against the per-block oracle."""
    Opt, kind, okind = OPT[opt]
    B, mb, nb = TRAJ
    A, b, x0 = plain_problem(B, mb, nb, TRAJ_SEED)
    n = B * nb
    lower, upper = np.full(n, -0.7), np.full(n, 0.8)
    ros = [block_oracle(A, b, x0, k, okind, iterations=25, lower=lower, upper=upper) for k in range(B)]
    assert all(ro.status == 0 for ro in ros)
    r = lsq.optimize_batched_(host_problem(A, b, x0), Opt(lsq.Cholesky()), iterations=25, lower=lower, upper=upper,
                              full_trace=True, ctx=ctx)
    assert np.all(r.minimizer >= lower) and np.all(r.minimizer <= upper)
    assert np.sum(r.minimizer == lower) + np.sum(r.minimizer == upper) > 0
    excused = 0
    for k in range(B):
        rb, ro = r.block(k), ros[k]
        assert np.all(rb.trace["x"] >= -0.7) and np.all(rb.trace["x"] <= 0.8)                 # every traced iterate is feasible
        same_counts(rb, ro, ("bounds", k))
        excused += compare_until_roundoff(rb, ro, ssr0=rb.ssr0) is not None
        assert np.max(np.abs(rb.minimizer - ro.minimizer)) <= 1e-8 * max(1.0, np.max(np.abs(ro.minimizer)))
        assert np.array_equal(rb.minimizer == -0.7, ro.minimizer == -0.7) and np.array_equal(rb.minimizer == 0.8, ro.minimizer == 0.8)
    assert excused <= 1
    with pytest.raises(lsq.ArgumentError) as e:                          # levenberg_marquardt.jl:51
        lsq.optimize_batched_(host_problem(A, b, np.full(n, 0.9)), Opt(lsq.Cholesky()), lower=lower, upper=upper, ctx=ctx)
    assert e.value.status == lsq._lib.EBOUNDS


# ------------------------------------------------------------------------------------------ 8. refusals at the C boundary
def test_refusals(ctx):
    import ctypes as C
    L = lsq.lib()
    A, b, x0 = plain_problem(4, 16, 8, 1)
    m, n = A.shape

    def call(Jd, okind, skind, hook=None):
        dx, dy = lsq.DeviceVector(ctx, Jd.n, np.zeros(Jd.n)), lsq.DeviceVector(ctx, Jd.m)
        st, _ = lsq.api._run_native_batched(ctx, okind, skind, Jd.h, (4, 16, 8), dx, dy, L.lsq_model_f(), L.lsq_model_g(), None,
                                            1e-8, 1e-8, 1e-8, 10, None, None, None, False, "x", options_hook=hook)
        return st, L.lsq_last_error().decode()

    LM, CH = lsq._lib.LEVENBERG_MARQUARDT, lsq._lib.CHOLESKY
    Jd = lsq.DeviceMatrix(ctx, A)
    for other in (lsq.DeviceMatrix(ctx, A.tocsc()), lsq.DeviceMatrix(ctx, np.zeros((m, n)))):
        st, msg = call(other, LM, CH)
        assert st == lsq._lib.EARG and "not block-diagonal" in msg
    st, msg = call(Jd, LM, lsq._lib.QR)
    assert st == lsq._lib.EARG and msg == "solver QR() is not available for sparse Jacobians. Choose between Cholesky() and LSMR()"
    st, msg = call(Jd, lsq._lib.DOGLEG, lsq._lib.LSMR)
    assert st == lsq._lib.EARG and "LSMR() is not available per block" in msg
    J65 = lsq.DeviceMatrix(ctx, make_A(2, 70, 65, 1))
    st, msg = call(J65, LM, CH)
    assert st == lsq._lib.EARG and "64" in msg and "65" in msg
    keep = []

    def hook_for(field, proto):
        def hook(opt):
            cb = proto(lambda *a: 0)
            keep.append(cb)
            setattr(opt, field, cb)
        return hook

    for field, proto, word in (("allreduce", lsq._lib.ALLREDUCE_CALLBACK, "sharded"),
                               ("row_allreduce", lsq._lib.ROW_ALLREDUCE_CALLBACK, "sharded"),
                               ("preconditioner", lsq._lib.PRECOND_CALLBACK, "preconditioner"),
                               ("precond_update", lsq._lib.PRECOND_UPDATE_CALLBACK, "preconditioner"),
                               ("precond_ldiv", lsq._lib.PRECOND_LDIV_CALLBACK, "preconditioner")):
        st, msg = call(Jd, LM, CH, hook_for(field, proto))
        assert st == lsq._lib.EARG and word in msg, (field, msg)
    # a device model needs a block-diagonal problem
    pr = lsq.synthetic.TanhProblem(64, 32, sparse=False, seed=1, ctx=ctx)
    with pytest.raises(lsq.ArgumentError):
        pr.optimize_batched()
    pr.close()
