"""Central-difference Jacobians on the device (csrc/lsq_fd.hip): lsq_fd_jacobian / fd_jacobian_ and the loops with g = NULL.

Everything here is compared BIT FOR BIT (np.array_equal on the raw values): the device routine and its host twins
(api._colored_difference_jacobian on block handles, api._central_difference_jacobian on dense ones) make the same f_ calls in
the same order on the same full vectors and take the same correctly rounded operations per entry, and f_ is the same host
function on both sides.  The loops are compared against THE SAME LOOP driven by the explicit twin as g_.

The batched problem: B = 37 exponential-decay fits r_i = a exp(-b t_i) + c - y_i (mb = 24, nb = 3), bounds on.  Block ZERO_BLOCK
starts at its minimizer (y is the model at x0, evaluated by f_'s own expression: residual exactly 0).  Block BAD_BLOCK becomes
non-finite: its rows are 1e-152 (A x) - y with x0 = 1e305, y ~ 1e158 and infinite bounds, so the first step towards
x* ~ 1e310 overflows; the refused trial point (x - dx) + dx is NaN and check_isfinite freezes the block (LSQ_ENONFINITE, index
0) while the others run on.  (A step can only overflow when |f| / |J| > 1.8e308 while J'J stays above the underflow threshold,
i.e. |J| > 1e-154 and |f| > 1e154: that block's own ssr is therefore Inf by construction.  x0 = 1e305 keeps 19 bits in the
differences f+ - f-, so its Jacobian has full rank.)  One trust region over the stacked problem (optimize_) cannot carry such
a block -- it ends the whole solve -- so those runs use the same BlockDiagonal shape and model with BAD_BLOCK an ordinary
decay fit."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from gpu_common import lsq

pytestmark = pytest.mark.gpu

api = lsq.api
L_ = lsq._lib


# ------------------------------------------------------------------------------------------------ operands
def special_x(n, seed):
    """+-0, negative, |x| = 1e8 (relative step), 1e-300 (absolute step) among ordinary entries."""
    x = np.random.default_rng(seed).uniform(-2.0, 2.0, n)
    for k, v in enumerate((0.0, -0.0, -3.5, 1e8, 1e-300, -1e8)):
        if k < n:
            x[(k * 7) % n] = v
    return x


def tanh_model(B, mb, nb, ng, seed):
    """r_{b,i} = sum_c A_{b,i,c} tanh(x_{b,c}) + (1 + tanh(x_{b,0})) sum_k W_{b,i,k} tanh(g_k): block-separable plus a border."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((B, mb, max(nb, 1)))
    W = rng.standard_normal((B, mb, max(ng, 1)))

    def f_(out, x):
        acc = np.zeros((B, mb))
        if nb:
            t = np.tanh(x[:B * nb].reshape(B, nb))
            acc = (A * t[:, None, :]).sum(axis=2)
        if ng:
            tg = np.tanh(x[B * nb:])
            lead = 1.0 + (np.tanh(x[:B * nb].reshape(B, nb)[:, 0]) if nb else np.zeros(B))
            acc = acc + lead[:, None] * (W * tg[None, None, :]).sum(axis=2)
        out[:] = acc.reshape(-1)

    return f_


def container(B, mb, nb, ng):
    return lsq.BorderedBlockDiagonal(B, mb, nb, ng) if ng else lsq.BlockDiagonal(B, mb, nb)


def twin_values(f_, B, mb, nb, ng, x):
    J = container(B, mb, nb, ng)
    J.data[:] = np.nan
    api._colored_difference_jacobian(f_, B * mb)(J, x)
    return J


BD_SHAPES = [(1, 1, 1), (5, 3, 3), (67, 33, 17), (3, 257, 16), (3, 1025, 5), (300, 8, 64), (2, 4, 65)]
BR_SHAPES = [(1, 2, 1, 1), (5, 7, 3, 2), (67, 33, 16, 5), (3, 257, 40, 24)]
DENSE_SHAPES = [(1, 1), (1000, 7), (63, 65)]


# ------------------------------------------------------------------------------------------------ 1. bits against the twins
@pytest.mark.parametrize("shape", BD_SHAPES + BR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fd_jacobian_bits_block_handles(ctx, shape):
    B, mb, nb = shape[:3]
    ng = shape[3] if len(shape) == 4 else 0
    n = B * nb + ng
    f_ = tanh_model(B, mb, nb, ng, 17)
    x = special_x(n, 23)
    ref = twin_values(f_, B, mb, nb, ng, x)
    assert np.all(np.isfinite(ref.data))
    Jd = lsq.DeviceMatrix(ctx, container(B, mb, nb, ng))
    try:
        calls = [0]

        def counted(out, xx):
            calls[0] += 1
            f_(out, xx)

        lsq.fd_jacobian_(Jd, x, counted)
        assert calls[0] == 2 * (nb + ng)
        got = Jd.values()
        bad = np.flatnonzero(got.view(np.uint64) != ref.data.view(np.uint64))
        assert bad.size == 0, (shape, bad[:8], got[bad[:8]], ref.data[bad[:8]])
    finally:
        Jd.free()


@pytest.mark.parametrize("shape", DENSE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fd_jacobian_bits_dense(ctx, shape):
    m, n = shape
    f_ = tanh_model(1, m, n, 0, 29)            # (one block: a dense m x n model)
    x = special_x(n, 31)
    ref = np.full((m, n), np.nan, order="F")
    api._central_difference_jacobian(f_, m)(ref, x)
    Jd = lsq.DeviceMatrix(ctx, np.zeros((m, n)))
    try:
        lsq.fd_jacobian_(Jd, lsq.DeviceVector(ctx, n, x), f_)
        got = Jd.values()
        assert np.array_equal(got.view(np.uint64), ref.reshape(-1, order="F").view(np.uint64)), shape
    finally:
        Jd.free()


# ------------------------------------------------------------------------------------------------ 2. determinism, refresh
@pytest.mark.parametrize("shape", [(67, 33, 17, 0), (5, 8, 3, 2), (67, 33, 16, 5)], ids=lambda s: "x".join(map(str, s)))
def test_determinism_and_refresh(ctx, shape):
    B, mb, nb, ng = shape
    m, n = B * mb, B * nb + ng
    f_ = tanh_model(B, mb, nb, ng, 41)
    x = np.random.default_rng(43).uniform(-1.5, 1.5, n)
    x[:3] = (0.0, -0.0, -2.0)
    ref = twin_values(f_, B, mb, nb, ng, x)
    Jd = lsq.DeviceMatrix(ctx, container(B, mb, nb, ng))            # (all zeros: every product of the old values is 0)
    try:
        lsq.fd_jacobian_(Jd, x, f_)
        first = Jd.values()
        assert np.array_equal(first, ref.data)
        # the handle's other layouts saw the new values: both products and the column sums
        D = ref.toarray()
        rng = np.random.default_rng(47)
        v, u = rng.standard_normal(n), rng.standard_normal(m)
        y = lsq.mul_(lsq.DeviceVector(ctx, m), Jd, lsq.DeviceVector(ctx, n, v)).get()
        z = lsq.mul_(lsq.DeviceVector(ctx, n), Jd, lsq.DeviceVector(ctx, m, u), trans=True).get()
        cs = lsq.colsumabs2_(lsq.DeviceVector(ctx, n), Jd).get()
        assert np.max(np.abs(D)) > 0.1
        assert np.max(np.abs(y - D @ v)) <= 1e-12 * np.max(np.abs(D) @ np.abs(v))
        assert np.max(np.abs(z - D.T @ u)) <= 1e-12 * np.max(np.abs(D.T) @ np.abs(u))
        assert np.max(np.abs(cs - (D * D).sum(axis=0))) <= 1e-12 * np.max((D * D).sum(axis=0))
        lsq.fd_jacobian_(Jd, x, f_)
        assert np.array_equal(Jd.values(), first)
        for jitter, serial in ((0, 1), (100, 0)):
            lsq.debug_set(jitter, serial)
            try:
                Jd.set_values(np.zeros(Jd.nnz))
                lsq.fd_jacobian_(Jd, x, f_)
                assert np.array_equal(Jd.values(), first), (jitter, serial)
            finally:
                lsq.debug_set(0, 0)
    finally:
        Jd.free()


# ------------------------------------------------------------------------------------------------ 3. loops
B_FIT, MB_FIT, NB_FIT = 37, 24, 3
ZERO_BLOCK, BAD_BLOCK = 4, 11
T_FIT = np.linspace(0.0, 4.0, MB_FIT)


def decay_rows(p):
    """(B, 3) parameters -> (B, mb) model values a exp(-b t) + c."""
    return p[:, 0][:, None] * np.exp(-(p[:, 1][:, None] * T_FIT[None, :])) + p[:, 2][:, None]


def decay_problem(bad=True, seed=5):
    """(f_, analytic g_, x0, lower, upper) of the batched problem of the module docstring."""
    B, mb, nb = B_FIT, MB_FIT, NB_FIT
    rng = np.random.default_rng(seed)
    ptrue = np.stack([rng.uniform(1.0, 3.0, B), rng.uniform(0.5, 1.5, B), rng.uniform(-0.5, 0.5, B)], axis=1)
    p0 = ptrue * (1.0 + 0.3 * rng.uniform(-1.0, 1.0, (B, 3))) + np.array([0.0, 0.0, 0.1])
    y = decay_rows(ptrue) + 0.01 * rng.standard_normal((B, mb))
    y[ZERO_BLOCK] = decay_rows(p0)[ZERO_BLOCK]
    lower = np.tile([0.0, 0.0, -10.0], B)
    upper = np.tile([100.0, 10.0, 10.0], B)
    Abad = rng.uniform(0.5, 1.5, (mb, nb))
    if bad:
        p0[BAD_BLOCK] = 1e305
        y[BAD_BLOCK] = 1e158 * rng.uniform(0.5, 1.5, mb)
        lower[BAD_BLOCK * nb:(BAD_BLOCK + 1) * nb] = -np.inf
        upper[BAD_BLOCK * nb:(BAD_BLOCK + 1) * nb] = np.inf

    def f_(out, x):
        p = x.reshape(B, nb)
        with np.errstate(all="ignore"):       # (the bad block's entries overflow in the decay expression, and are replaced)
            r = decay_rows(p) - y
            if bad:
                xb = p[BAD_BLOCK]
                r[BAD_BLOCK] = 1e-152 * (Abad[:, 0] * xb[0] + Abad[:, 1] * xb[1] + Abad[:, 2] * xb[2]) - y[BAD_BLOCK]
        out[:] = r.reshape(-1)

    def g_(J, x):       # the analytic Jacobian of the decay fits (only used without the bad block)
        p = x.reshape(B, nb)
        e = np.exp(-(p[:, 1][:, None] * T_FIT[None, :]))
        blocks = J.data.reshape(B, nb, mb)
        blocks[:, 0, :] = e
        blocks[:, 1, :] = -p[:, 0][:, None] * T_FIT[None, :] * e
        blocks[:, 2, :] = 1.0

    return f_, g_, p0.reshape(-1).copy(), lower, upper


def fit_nls(f_, x0, g_="device"):
    """g_ = "device": left to the default (central differences on the device); "twin": the explicit coloured host twin."""
    m = B_FIT * MB_FIT
    kw = {} if g_ == "device" else {"g_": api._colored_difference_jacobian(f_, m) if g_ == "twin" else g_}
    nls = lsq.LeastSquaresProblem(x=x0.copy(), y=np.zeros(m), f_=f_, J=lsq.BlockDiagonal(B_FIT, MB_FIT, NB_FIT), **kw)
    assert api._device_fd(nls) == (g_ == "device")
    return nls


def same(a, b, label):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (label, a.shape, b.shape)
    if a.dtype.kind == "f":
        assert np.array_equal(a, b, equal_nan=True), (label, np.flatnonzero(~((a == b) | (np.isnan(a) & np.isnan(b))).reshape(-1))[:8])
    else:
        assert np.array_equal(a, b), label


BATCHED_FIELDS = ("minimizer", "ssr", "ssr0", "iterations", "converged", "x_converged", "f_converged", "g_converged", "f_calls",
                  "g_calls", "mul_calls", "status", "info")
SINGLE_FIELDS = ("minimizer", "ssr", "iterations", "converged", "x_converged", "f_converged", "g_converged", "f_calls", "g_calls",
                 "mul_calls")


def same_batched(rd, rt, label):
    assert rd.outer_iterations == rt.outer_iterations, label
    for k in BATCHED_FIELDS:
        same(getattr(rd, k), getattr(rt, k), (label, k))
    for k in rt.trace:
        same(rd.trace[k], rt.trace[k], (label, "trace", k))


def same_single(rd, rt, label):
    for k in SINGLE_FIELDS:
        same(getattr(rd, k), getattr(rt, k), (label, k))
    for k in rt.trace:
        same(rd.trace[k], rt.trace[k], (label, "trace", k))


SOLVERS = {"cholesky": lsq.Cholesky, "blockqr": lsq.BlockQR}
OPTIMIZERS = {"lm": lsq.LevenbergMarquardt, "dogleg": lsq.Dogleg}


@pytest.mark.parametrize("solver", ["cholesky", "blockqr"])
@pytest.mark.parametrize("opt", ["lm", "dogleg"])
def test_batched_loop_bits(ctx, opt, solver):
    f_, _, x0, lower, upper = decay_problem(bad=True)
    run = lambda nls: lsq.optimize_batched_(nls, OPTIMIZERS[opt](SOLVERS[solver]()), iterations=40, lower=lower, upper=upper,
                                            full_trace=True, ctx=ctx)
    nd, nt = fit_nls(f_, x0, "device"), fit_nls(f_, x0, "twin")
    rd, rt = run(nd), run(nt)
    print(opt, solver, "iterations", rd.iterations.tolist(), "status", rd.status.tolist())
    same_batched(rd, rt, (opt, solver))
    same(nd.J.data, nt.J.data, "J of the last evaluation")
    same(nd.y, nt.y, "y")
    assert rd.status[BAD_BLOCK] == L_.ENONFINITE and rd.info[BAD_BLOCK] == 0
    others = [b for b in range(B_FIT) if b != BAD_BLOCK]
    assert np.all(rd.status[others] == 0) and np.all(rd.converged[others] == 1)
    assert rd.iterations[BAD_BLOCK] < rd.outer_iterations             # the others went on after it was frozen
    assert rd.iterations[ZERO_BLOCK] == 1 and rd.ssr[ZERO_BLOCK] == 0.0 and rd.g_calls[ZERO_BLOCK] == 1
    assert np.array_equal(rd.minimizer[ZERO_BLOCK * NB_FIT:(ZERO_BLOCK + 1) * NB_FIT], x0[ZERO_BLOCK * NB_FIT:(ZERO_BLOCK + 1) * NB_FIT])
    assert len(set(rd.iterations[others].tolist())) > 1                # the fits really differ


def test_batched_counts_exclude_the_differences(ctx):
    """f_calls[b] is what the optimizer itself evaluated: equal to the run with the analytic g_ of the same model wherever
    both take the same number of iterations (and in any case equal to the twin-driven run's, test_batched_loop_bits)."""
    f_, g_, x0, lower, upper = decay_problem(bad=False)
    calls = [0]

    def counted(out, x):
        calls[0] += 1
        f_(out, x)

    run = lambda nls: lsq.optimize_batched_(nls, lsq.LevenbergMarquardt(lsq.Cholesky()), iterations=40, lower=lower, upper=upper, ctx=ctx)
    rd = run(fit_nls(counted, x0, "device"))
    total = calls[0]
    ra = run(fit_nls(f_, x0, g_))
    eq = np.flatnonzero(rd.iterations == ra.iterations)
    print("same iteration count on", eq.size, "of", B_FIT, "blocks; f_ was called", total, "times")
    assert eq.size > 0
    assert np.array_equal(rd.f_calls[eq], ra.f_calls[eq])
    # the host function saw the uncounted ones: 2 nb per Jacobian of the batch, one Jacobian per pass that wanted any
    assert total > int(rd.f_calls.max()) and (total - rd.outer_iterations - 1) % (2 * NB_FIT) == 0


@pytest.mark.parametrize("solver", ["cholesky", "lsmr"])
def test_single_trust_region_on_blockdiag(ctx, solver):
    f_, _, x0, lower, upper = decay_problem(bad=False)
    S = {"cholesky": lsq.Cholesky, "lsmr": lsq.LSMR}[solver]
    run = lambda nls: lsq.optimize_(nls, lsq.LevenbergMarquardt(S()), iterations=40, lower=lower, upper=upper, full_trace=True, ctx=ctx)
    nd, nt = fit_nls(f_, x0, "device"), fit_nls(f_, x0, "twin")
    rd, rt = run(nd), run(nt)
    print(solver, "iterations", rd.iterations, "ssr", rd.ssr, "calls", rd.f_calls, rd.g_calls, rd.mul_calls)
    same_single(rd, rt, solver)
    same(nd.J.data, nt.J.data, "J of the last evaluation")
    assert rd.converged and rd.g_calls >= 2


def test_single_trust_region_on_bordered(ctx):
    B, mb, nb, ng = 9, 12, 2, 2
    m, n = B * mb, B * nb + ng
    t = np.linspace(0.0, 3.0, mb)
    rng = np.random.default_rng(8)
    loc = np.stack([rng.uniform(1.0, 2.0, B), rng.uniform(-0.5, 0.5, B)], axis=1)
    glob = np.array([0.8, 0.3])

    def rows(lc, gl):
        return lc[:, 0][:, None] * np.exp(-(gl[0] * t[None, :])) + lc[:, 1][:, None] + gl[1] * t[None, :]

    y = rows(loc, glob) + 0.01 * rng.standard_normal((B, mb))

    def f_(out, x):
        out[:] = (rows(x[:B * nb].reshape(B, nb), x[B * nb:]) - y).reshape(-1)

    x0 = np.concatenate([(loc * 1.2).reshape(-1), [1.0, 0.0]])

    def run(device):
        kw = {} if device else {"g_": api._colored_difference_jacobian(f_, m)}
        nls = lsq.LeastSquaresProblem(x=x0.copy(), y=np.zeros(m), f_=f_, J=lsq.BorderedBlockDiagonal(B, mb, nb, ng), **kw)
        assert api._device_fd(nls) == device
        return nls, lsq.optimize_(nls, lsq.LevenbergMarquardt(lsq.Cholesky()), iterations=40, full_trace=True, ctx=ctx)

    (nd, rd), (nt, rt) = run(True), run(False)
    print("bordered: iterations", rd.iterations, "ssr", rd.ssr)
    same_single(rd, rt, "bordered")
    same(nd.J.data, nt.J.data, "J of the last evaluation")
    assert rd.converged and rd.g_calls >= 2


def host_f_callback(ctx, f_, m, n, err):
    xh, yh = np.zeros(n), np.zeros(m)

    def _f(d_out, d_x, _):
        try:
            api.check(lsq.lib().lsq_d2h(ctx.h, xh.ctypes.data_as(C.c_void_p), d_x, n * 8))
            f_(yh, xh)
            api.check(lsq.lib().lsq_h2d(ctx.h, d_out, yh.ctypes.data_as(C.c_void_p), m * 8))
            return 0
        except Exception as e:
            err.append(e)
            return 1

    return L_.F_CALLBACK(_f)


@pytest.mark.parametrize("opt,solver", [("dogleg", lsq.QR), ("lm", lsq.Cholesky)])
def test_lsq_optimize_null_g_dense(ctx, opt, solver):
    """lsq_optimize called directly with a NULL g on a dense 40 x 3 handle against optimize_ with the dense host twin."""
    m, n = 40, 3
    t = np.linspace(0.0, 4.0, m)
    rng = np.random.default_rng(12)
    y = 2.0 * np.exp(-0.7 * t) + 0.3 + 0.01 * rng.standard_normal(m)

    def f_(out, x):
        out[:] = x[0] * np.exp(-(x[1] * t)) + x[2] - y

    x0 = np.array([1.0, 1.0, 0.0])
    Opt = OPTIMIZERS[opt]
    nls = lsq.LeastSquaresProblem(x=x0.copy(), y=np.zeros(m), f_=f_)          # no J, no g_: the dense host twin
    assert not api._device_fd(nls)
    rt = lsq.optimize_(nls, Opt(solver()), iterations=50, full_trace=True, ctx=ctx)
    err = []
    F = host_f_callback(ctx, f_, m, n, err)
    Jd = lsq.DeviceMatrix(ctx, np.zeros((m, n)))
    dx, dy = lsq.DeviceVector(ctx, n, x0), lsq.DeviceVector(ctx, m)
    try:
        st, res, tr = api._run_native(ctx, Opt.kind, solver.kind, Jd, dx, dy, F, L_.G_CALLBACK(), None, 1e-8, 1e-8, 1e-8, 50,
                                      None, (), (), True, n)
        assert not err and st == 0, (st, err)
        same(dx.get(), rt.minimizer, "minimizer")
        same(dy.get(), nls.y, "y")
        assert (res.ssr, res.iterations, res.converged, res.x_converged, res.f_converged, res.g_converged, res.f_calls,
                res.g_calls, res.mul_calls, res.status) == \
               (rt.ssr, rt.iterations, int(rt.converged), int(rt.x_converged), int(rt.f_converged), int(rt.g_converged),
                rt.f_calls, rt.g_calls, rt.mul_calls, 0)
        for k in rt.trace:
            same(tr[k], rt.trace[k], ("trace", k))
        same(Jd.values(), np.asarray(nls.J).reshape(-1, order="F"), "J of the last evaluation")
        assert rt.converged and rt.g_calls >= 2
    finally:
        Jd.free()


def test_allocated_problem_twice(ctx):
    f_, _, x0, lower, upper = decay_problem(bad=False)
    nlsa = lsq.LeastSquaresProblemAllocated(fit_nls(f_, x0, "device"), lsq.LevenbergMarquardt(lsq.Cholesky()), ctx=ctx)
    try:
        assert api._device_fd(nlsa)
        out = []
        for _ in range(2):
            nlsa.x[:] = x0
            nlsa.y[:] = 0.0
            r = lsq.optimize_(nlsa, iterations=40, lower=lower, upper=upper, full_trace=True)
            out.append((r.minimizer.copy(), r.ssr, r.iterations, r.f_calls, r.g_calls, r.mul_calls, {k: v.copy() for k, v in r.trace.items()},
                        nlsa.J.data.copy()))
        a, b = out
        same(a[0], b[0], "minimizer")
        assert a[1:6] == b[1:6]
        for k in a[6]:
            same(a[6][k], b[6][k], ("trace", k))
        same(a[7], b[7], "J")
        rt = lsq.optimize_(fit_nls(f_, x0, "twin"), lsq.LevenbergMarquardt(lsq.Cholesky()), iterations=40, lower=lower, upper=upper,
                           full_trace=True, ctx=ctx)
        same(a[0], rt.minimizer, "minimizer against the twin-driven run")
        assert a[1:6] == (rt.ssr, rt.iterations, rt.f_calls, rt.g_calls, rt.mul_calls)
    finally:
        nlsa.free()


# ------------------------------------------------------------------------------------------------ 4. refusals and errors
def test_refusals(ctx):
    f_ = lambda out, x: out.__setitem__(slice(None), 0.0)
    S = sp.random(12, 5, density=0.5, format="csc", random_state=np.random.default_rng(1))
    Jc = lsq.DeviceMatrix(ctx, S)
    try:
        with pytest.raises(lsq.ArgumentError):
            lsq.fd_jacobian_(Jc, np.zeros(5), f_)
        # lsq_optimize with a NULL g on a plain CSC handle
        err = []
        F = host_f_callback(ctx, f_, 12, 5, err)
        st, res, _ = api._run_native(ctx, L_.LEVENBERG_MARQUARDT, L_.LSMR, Jc, lsq.DeviceVector(ctx, 5), lsq.DeviceVector(ctx, 12), F,
                                     L_.G_CALLBACK(), None, 1e-8, 1e-8, 1e-8, 10, None, (), (), False, 5)
        assert st == L_.EARG and res.status == L_.EARG and not err
        assert b"colouring" in lsq.lib().lsq_last_error()
    finally:
        Jc.free()
    op = lsq.DeviceOperator(ctx, 6, 3, lambda t, x, out: None, lambda out: None)
    try:
        with pytest.raises(lsq.ArgumentError):
            lsq.fd_jacobian_(op, np.zeros(3), f_)
    finally:
        op.free()
    Jb = lsq.DeviceMatrix(ctx, lsq.BlockDiagonal(3, 4, 2))
    s = lsq.DeviceVector(ctx, 6, np.ones(6))
    try:
        Jb.set_colscale(s)
        with pytest.raises(lsq.ArgumentError):
            lsq.fd_jacobian_(Jb, np.zeros(6), f_)
        Jb.set_colscale(None)
        lsq.fd_jacobian_(Jb, np.zeros(6), f_)            # the plain handle again: accepted
    finally:
        Jb.free()
    # a plain CSC Jacobian without g_ still raises at the first g!
    nls = lsq.LeastSquaresProblem(x=np.ones(5), y=np.zeros(12), f_=f_, J=S)
    with pytest.raises(lsq.ArgumentError):
        lsq.optimize_(nls, lsq.LevenbergMarquardt(lsq.LSMR()), ctx=ctx)


class Boom(Exception):
    pass


def test_f_that_raises_inside_a_colour(ctx):
    B, mb, nb, ng = 5, 7, 3, 2
    f_ = tanh_model(B, mb, nb, ng, 3)
    x = special_x(B * nb + ng, 4)
    calls = [0]

    def flaky(out, xx):
        calls[0] += 1
        if calls[0] == 4:                 # f- of the second colour
            raise Boom("inside colour 1")
        f_(out, xx)

    Jd = lsq.DeviceMatrix(ctx, container(B, mb, nb, ng))
    try:
        with pytest.raises(Boom):
            lsq.fd_jacobian_(Jd, x, flaky)
        assert calls[0] == 4
        lsq.fd_jacobian_(Jd, x, f_)       # the handle is usable, and nothing of the aborted call is left in its work vectors
        assert np.array_equal(Jd.values(), twin_values(f_, B, mb, nb, ng, x).data)
    finally:
        Jd.free()
