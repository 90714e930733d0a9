"""Coloured central differences on general sparse patterns, on the device (csrc/lsq_fd.hip: lsq_mat_set_fd_colouring, then
lsq_fd_jacobian / fd_jacobian_ and the loops with g = NULL on a plain CSC handle).

Everything is compared BIT FOR BIT: the device routine and its host twin (api._sparse_colored_difference_jacobian) make the
same f_ calls in the same order on the same full vectors and take the same correctly rounded operations per stored entry, and
f_ is the same host function on both sides.  The loops are compared against THE SAME LOOP driven by the explicit twin as g_.
Patterns, models and helpers: fd_sparse_common.py."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import lsq_amd as lsq

import fd_sparse_common as FS

pytestmark = pytest.mark.gpu

api = lsq.api
L_ = lsq._lib

PATTERNS = dict(FS.host_patterns())
PATTERNS["tall3000x9"] = FS.tall_column_pattern()
PATTERNS["perm2100"] = FS.permutation_pattern()


def twin_values(f_, S, colour, x):
    J = S.copy()
    J.data[:] = np.nan
    api._sparse_colored_difference_jacobian(f_, S.shape[0], colour)(J, x)
    return J.data.copy()


def coloured_handle(ctx, S, colours=None):
    Jd = lsq.DeviceMatrix(ctx, S)
    Jd.set_fd_colouring(colours)
    return Jd


# ------------------------------------------------------------------------------------------------ 1. bits against the twin
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_fd_jacobian_bits(ctx, name):
    S = PATTERNS[name]
    m, n = S.shape
    f_ = FS.poly_rowwise_model(S, 17)
    x = FS.special_x(n, 23)
    greedy, nc = lsq.greedy_colouring(S)
    ref = twin_values(f_, S, greedy, x)
    assert np.all(np.isfinite(ref))
    Jd = lsq.DeviceMatrix(ctx, S)
    Ju = lsq.DeviceMatrix(ctx, S)
    try:
        assert Jd.fd_colouring() == (None, 0)
        assert Jd.set_fd_colouring() == nc
        got_colour, got_nc = Jd.fd_colouring()
        assert got_nc == nc and np.array_equal(got_colour, greedy)
        calls = [0]

        def counted(out, xx):
            calls[0] += 1
            f_(out, xx)

        Jd.set_values(np.full(Jd.nnz, np.nan))                     # every stored entry must be written
        lsq.fd_jacobian_(Jd, x, counted)
        assert calls[0] == 2 * nc
        FS.same_bits(Jd.values(), ref, name)
        # a colouring of the user's own (the greedy colours relabelled in reverse): other calls of f_, the same bits
        hand = (nc - 1 - greedy).astype(np.int32)
        assert Ju.set_fd_colouring(hand) == nc
        assert np.array_equal(Ju.fd_colouring()[0], hand)
        lsq.fd_jacobian_(Ju, lsq.DeviceVector(ctx, n, x), f_)
        FS.same_bits(Ju.values(), ref, (name, "user-supplied"))
        FS.same_bits(twin_values(f_, S, hand, x), ref, (name, "twin, user-supplied"))
    finally:
        Jd.free()
        Ju.free()


def test_blockdiag_as_csc_equals_the_blockdiagonal_handle(ctx):
    B, mb, nb = 5, 7, 3
    S = PATTERNS["blockdiag5x7x3"]
    f_ = FS.poly_rowwise_model(S, 31)
    x = FS.special_x(B * nb, 37)
    Jc = coloured_handle(ctx, S)
    Jb = lsq.DeviceMatrix(ctx, lsq.BlockDiagonal(B, mb, nb))
    try:
        assert np.array_equal(Jc.fd_colouring()[0], np.arange(B * nb) % nb)
        lsq.fd_jacobian_(Jc, x, f_)
        lsq.fd_jacobian_(Jb, x, f_)
        FS.same_bits(Jc.values(), Jb.values())                    # (the value order is the same: blocks column-major)
    finally:
        Jc.free()
        Jb.free()


# ------------------------------------------------------------------------------------------------ 2. determinism
@pytest.mark.parametrize("name", ["random61x23s2", "tall3000x9", "perm2100"])
def test_same_bits_serial_and_under_jitter(ctx, name):
    S = PATTERNS[name]
    f_ = FS.poly_rowwise_model(S, 41)
    x = FS.special_x(S.shape[1], 43)
    Jd = coloured_handle(ctx, S)
    try:
        lsq.fd_jacobian_(Jd, x, f_)
        first = Jd.values()
        FS.same_bits(first, twin_values(f_, S, Jd.fd_colouring()[0], x))
        for jitter, serial in ((0, 1), (100, 0)):
            lsq.debug_set(jitter, serial)
            try:
                Jd.set_values(np.zeros(Jd.nnz))
                lsq.fd_jacobian_(Jd, x, f_)
                FS.same_bits(Jd.values(), first, (name, jitter, serial))
            finally:
                lsq.debug_set(0, 0)
    finally:
        Jd.free()


# ------------------------------------------------------------------------------------------------ 3. the other layouts
def products(ctx, Jd, v, u):
    y = lsq.mul_(lsq.DeviceVector(ctx, Jd.m), Jd, lsq.DeviceVector(ctx, Jd.n, v)).get()
    z = lsq.mul_(lsq.DeviceVector(ctx, Jd.n), Jd, lsq.DeviceVector(ctx, Jd.m, u), trans=True).get()
    return y, z


@pytest.mark.parametrize("shape,force", [((61, 23), False), ((4000, 129), True)], ids=["61x23", "4000x129-sliced"])
def test_other_layouts_are_refreshed(ctx, monkeypatch, shape, force):
    if force:
        monkeypatch.setenv("LSQ_SELL_FORCE", "1")                  # (read when a handle is created: sliced layouts for both)
    m, n = shape
    S = FS.random_pattern(7, m, n, 0.15 if m < 100 else 0.03)
    f_ = FS.poly_rowwise_model(S, 53)
    x = np.random.default_rng(59).uniform(-1.5, 1.5, n)
    Jd = coloured_handle(ctx, S)
    Jf = lsq.DeviceMatrix(ctx, S)
    try:
        rng = np.random.default_rng(61)
        v, u = rng.standard_normal(n), rng.standard_normal(m)
        y0, z0 = products(ctx, Jd, v, u)                          # (the pattern's ones: the mirrors hold something else first)
        lsq.fd_jacobian_(Jd, x, f_)
        ref = twin_values(f_, S, Jd.fd_colouring()[0], x)
        FS.same_bits(Jd.values(), ref)
        Jf.set_values(ref)
        y, z = products(ctx, Jd, v, u)
        yf, zf = products(ctx, Jf, v, u)
        assert not np.array_equal(y, y0) and not np.array_equal(z, z0)
        FS.same_bits(y, yf, "J v")
        FS.same_bits(z, zf, "J' u")
        FS.same_bits(lsq.colsumabs2_(lsq.DeviceVector(ctx, n), Jd).get(), lsq.colsumabs2_(lsq.DeviceVector(ctx, n), Jf).get(), "colsumabs2")
    finally:
        Jd.free()
        Jf.free()


# ------------------------------------------------------------------------------------------------ 4. the loops
FIT_S = FS.random_pattern(11, 61, 23, 0.2)
SINGLE_FIELDS = ("minimizer", "ssr", "iterations", "converged", "x_converged", "f_converged", "g_converged", "f_calls", "g_calls",
                 "mul_calls")


def fit_nls(f_, x0, how, colouring=None):
    m = FIT_S.shape[0]
    if how == "device":
        nls = lsq.LeastSquaresProblem(x=x0.copy(), y=np.zeros(m), f_=f_, J=FIT_S.copy(), autodiff="central_coloured", colouring=colouring)
    else:
        colour = colouring if colouring is not None else lsq.greedy_colouring(FIT_S)[0]
        nls = lsq.LeastSquaresProblem(x=x0.copy(), y=np.zeros(m), f_=f_, J=FIT_S.copy(),
                                      g_=api._sparse_colored_difference_jacobian(f_, m, colour))
    assert api._device_fd(nls) == (how == "device")
    return nls


def same(a, b, label):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (label, a.shape, b.shape)
    assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), label


def same_single(rd, rt, label):
    for k in SINGLE_FIELDS:
        same(getattr(rd, k), getattr(rt, k), (label, k))
    assert set(rd.trace) == set(rt.trace)
    for k in rt.trace:
        same(rd.trace[k], rt.trace[k], (label, "trace", k))


@pytest.mark.parametrize("opt,bounds", [("lm", False), ("dogleg", False), ("lm", True)])
def test_optimize_against_the_twin_driven_loop(ctx, opt, bounds):
    f_, _, x0, x_true = FS.tanh_fit_problem(FIT_S, 5)
    n = len(x0)
    kw = {}
    if bounds:          # some of them active at the solution
        kw = {"lower": np.minimum(x0, np.where(np.arange(n) % 3 == 0, x_true + 0.05, -2.0)),
              "upper": np.maximum(x0, np.where(np.arange(n) % 3 == 1, x_true - 0.05, 2.0))}
    Opt = {"lm": lsq.LevenbergMarquardt, "dogleg": lsq.Dogleg}[opt]
    run = lambda nls: lsq.optimize_(nls, Opt(lsq.LSMR()), iterations=40, full_trace=True, ctx=ctx, **kw)
    nd, nt = fit_nls(f_, x0, "device"), fit_nls(f_, x0, "twin")
    rd, rt = run(nd), run(nt)
    print(opt, bounds, "iterations", rd.iterations, "ssr", rd.ssr, "calls", rd.f_calls, rd.g_calls, rd.mul_calls)
    same_single(rd, rt, (opt, bounds))
    same(nd.J.data, nt.J.data, "J of the last evaluation")
    same(nd.y, nt.y, "y")
    assert rd.g_calls >= 2 and (rd.converged or bounds)


def test_counts_exclude_the_differences(ctx):
    f_, _, x0, _ = FS.tanh_fit_problem(FIT_S, 5)
    calls = [0]

    def counted(out, x):
        calls[0] += 1
        f_(out, x)

    nc = lsq.greedy_colouring(FIT_S)[1]
    r = lsq.optimize_(fit_nls(counted, x0, "device"), lsq.LevenbergMarquardt(lsq.LSMR()), iterations=40, ctx=ctx)
    print("f_ was called", calls[0], "times; f_calls", r.f_calls, "g_calls", r.g_calls, "colours", nc)
    # f_calls is what the optimizer itself evaluated (equal to the twin-driven run's, above): the 2 nc evaluations of every
    # Jacobian reached the host function on top of it
    assert r.g_calls >= 2 and calls[0] >= r.f_calls + 2 * nc * r.g_calls


def test_allocated_problem_twice(ctx):
    f_, _, x0, _ = FS.tanh_fit_problem(FIT_S, 6)
    nlsa = lsq.LeastSquaresProblemAllocated(fit_nls(f_, x0, "device"), lsq.LevenbergMarquardt(lsq.LSMR()), ctx=ctx)
    try:
        assert api._device_fd(nlsa)
        out = []
        for _ in range(2):
            nlsa.x[:] = x0
            nlsa.y[:] = 0.0
            r = lsq.optimize_(nlsa, iterations=40, full_trace=True)
            out.append((r.minimizer.copy(), (r.ssr, r.iterations, r.f_calls, r.g_calls, r.mul_calls),
                        {k: v.copy() for k, v in r.trace.items()}, nlsa.J.data.copy()))
        a, b = out
        same(a[0], b[0], "minimizer")
        assert a[1] == b[1]
        for k in a[2]:
            same(a[2][k], b[2][k], ("trace", k))
        same(a[3], b[3], "J")
        assert nlsa._Jd.fd_colouring()[1] == lsq.greedy_colouring(FIT_S)[1]
        rt = lsq.optimize_(fit_nls(f_, x0, "twin"), lsq.LevenbergMarquardt(lsq.LSMR()), iterations=40, full_trace=True, ctx=ctx)
        same(a[0], rt.minimizer, "minimizer against the twin-driven run")
        assert a[1] == (rt.ssr, rt.iterations, rt.f_calls, rt.g_calls, rt.mul_calls)
        for k in rt.trace:
            same(a[2][k], rt.trace[k], ("trace against the twin-driven run", k))
    finally:
        nlsa.free()


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


def test_lsq_optimize_null_g(ctx):
    """lsq_optimize called directly with a NULL g on a coloured CSC handle against optimize_ with the explicit twin."""
    m, n = FIT_S.shape
    f_, _, x0, _ = FS.tanh_fit_problem(FIT_S, 7)
    nls = fit_nls(f_, x0, "twin")
    rt = lsq.optimize_(nls, lsq.LevenbergMarquardt(lsq.LSMR()), iterations=40, full_trace=True, ctx=ctx)
    err = []
    F = host_f_callback(ctx, f_, m, n, err)
    Jd = coloured_handle(ctx, FIT_S)
    dx, dy = lsq.DeviceVector(ctx, n, x0), lsq.DeviceVector(ctx, m)
    try:
        st, res, tr = api._run_native(ctx, L_.LEVENBERG_MARQUARDT, L_.LSMR, Jd, dx, dy, F, L_.G_CALLBACK(), None, 1e-8, 1e-8, 1e-8, 40,
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
        same(Jd.values(), nls.J.data, "J of the last evaluation")
        assert rt.converged and rt.g_calls >= 2
    finally:
        Jd.free()


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals(ctx):
    zero = lambda out, x: out.__setitem__(slice(None), 0.0)
    others = [lsq.DeviceMatrix(ctx, np.zeros((4, 3))), lsq.DeviceMatrix(ctx, lsq.BlockDiagonal(3, 4, 2)),
              lsq.DeviceMatrix(ctx, lsq.BorderedBlockDiagonal(3, 4, 2, 1)),
              lsq.DeviceOperator(ctx, 6, 3, lambda t, x, out: None, lambda out: None)]
    try:
        for h, word in zip(others, (b"dense", b"block-diagonal", b"bordered", b"operator")):
            st = lsq.lib().lsq_mat_set_fd_colouring(h.h, None, None)
            assert st == L_.EARG and word in lsq.lib().lsq_last_error(), word
        for h in others[:3]:
            with pytest.raises(lsq.ArgumentError):
                h.set_fd_colouring()
            assert h.fd_colouring() == (None, 0)
    finally:
        for h in others:
            h.free()
    S = PATTERNS["arrow9"]
    Jc = lsq.DeviceMatrix(ctx, S)
    try:
        assert Jc.fd_colouring() == (None, 0)                      # nothing attached: 0 colours, and still refused
        with pytest.raises(lsq.ArgumentError, match="lsq_mat_set_fd_colouring"):
            lsq.fd_jacobian_(Jc, np.zeros(9), zero)
        assert b"colouring" in lsq.lib().lsq_last_error()
        clash = np.arange(9, dtype=np.int32)
        clash[[2, 5]] = [5, 5]
        clash[8] = 2                                               # no gap, nothing negative: only row 0 is wrong
        with pytest.raises(lsq.ArgumentError, match="row 0 .*columns 2 and 5"):
            Jc.set_fd_colouring(clash)
        negative = np.arange(9, dtype=np.int32)
        negative[4] = -1
        with pytest.raises(lsq.ArgumentError, match="negative"):
            Jc.set_fd_colouring(negative)
        with pytest.raises(lsq.ArgumentError, match="gap"):
            Jc.set_fd_colouring(np.arange(9, dtype=np.int32) + 1)  # colour 0 unused
        with pytest.raises(lsq.ArgumentError, match="gap"):
            Jc.set_fd_colouring(np.arange(9, dtype=np.int32) * 3)
        with pytest.raises(lsq.ArgumentError):
            Jc.set_fd_colouring(np.arange(8, dtype=np.int32))      # wrong length, refused before the library sees it
        assert Jc.fd_colouring() == (None, 0)                      # a refused colouring leaves the handle as it was
        assert Jc.set_fd_colouring() == 9
        # a column scale: refused as on any handle, accepted again once it is removed
        s = lsq.DeviceVector(ctx, 9, np.ones(9))
        Jc.set_colscale(s)
        with pytest.raises(lsq.ArgumentError):
            lsq.fd_jacobian_(Jc, np.zeros(9), zero)
        Jc.set_colscale(None)
        assert Jc.fd_colouring()[1] == 9                           # (the scale did not disturb the colouring)
        lsq.fd_jacobian_(Jc, np.zeros(9), zero)
        assert np.array_equal(Jc.values(), np.zeros(Jc.nnz))
    finally:
        Jc.free()


# ------------------------------------------------------------------------------------------------ 6. an f_ that raises
class Boom(Exception):
    pass


def test_f_that_raises_inside_the_second_colour(ctx):
    S = PATTERNS["random61x23s3"]
    m, n = S.shape
    f_ = FS.poly_rowwise_model(S, 3)
    x = FS.special_x(n, 4)
    calls = [0]

    def flaky(out, xx):
        calls[0] += 1
        if calls[0] == 4:                 # f- of the second colour
            raise Boom("inside colour 1")
        f_(out, xx)

    Jd = coloured_handle(ctx, S)
    Jf = lsq.DeviceMatrix(ctx, S)
    try:
        assert Jd.fd_colouring()[1] >= 3
        with pytest.raises(Boom):
            lsq.fd_jacobian_(Jd, x, flaky)
        assert calls[0] == 4
        # some columns are new, some are not: the layouts of the handle agree with each other
        rng = np.random.default_rng(9)
        v, u = rng.standard_normal(n), rng.standard_normal(m)
        Jf.set_values(Jd.values())
        for a, b in zip(products(ctx, Jd, v, u), products(ctx, Jf, v, u)):
            FS.same_bits(a, b, "after the aborted call")
        # the next call is clean: nothing of the aborted one is left in the work vectors
        Jf.set_fd_colouring()
        lsq.fd_jacobian_(Jd, x, f_)
        lsq.fd_jacobian_(Jf, x, f_)
        FS.same_bits(Jd.values(), Jf.values())
        FS.same_bits(Jd.values(), twin_values(f_, S, Jd.fd_colouring()[0], x))
    finally:
        Jd.free()
        Jf.free()


# ------------------------------------------------------------------------------------------------ 7. replacing the colouring
def test_replacing_the_colouring_on_a_live_handle(ctx):
    S = PATTERNS["random61x23s4"]
    n = S.shape[1]
    f_ = FS.poly_rowwise_model(S, 13)
    x = FS.special_x(n, 14)
    Jd = coloured_handle(ctx, S)
    try:
        nc = Jd.fd_colouring()[1]
        lsq.fd_jacobian_(Jd, x, f_)
        first = Jd.values()
        calls = [0]

        def counted(out, xx):
            calls[0] += 1
            f_(out, xx)

        assert Jd.set_fd_colouring(np.arange(n, dtype=np.int32)) == n > nc
        Jd.set_values(np.zeros(Jd.nnz))                            # (uploading values does not disturb the colouring)
        assert Jd.fd_colouring()[1] == n
        lsq.fd_jacobian_(Jd, x, counted)
        assert calls[0] == 2 * n
        FS.same_bits(Jd.values(), first)
    finally:
        Jd.free()
