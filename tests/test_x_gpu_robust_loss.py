"""Robust loss tier on the device (tests/robust_loss_common.py has the cases and the references; tests/test_robust_loss_host.py
certifies them on the CPU).

  * lsq_mat_scale_rows, bit for bit against V * w[row] on every handle kind and layout, with 0, -1, 2^-600 and NaN among the
    factors; every reader afterwards against a fresh handle holding the scaled values; mixed with the other mutation routes
    in both orders; under the serial and jitter debug modes; its refusals.
  * lsq_loss_eval against the numpy twin (lsq_amd.loss_transform): the twin's bits for linear / huber / soft_l1, the accuracy
    rule for cauchy (e_ref: the twin's own error against the longdouble reference); statistics; refusals of lsq_loss_create.
  * every loop with loss= against the SAME loop driven by lsq_amd.robust_twin host callbacks: every field of the result, x, y,
    the Jacobian values and the trace, bit for bit.
  * limiting cases, the gradient of the robust cost at the result, covariance on the live handle, failures."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import accuracy_common as ac
import handle_state_common as H
import robust_loss_common as R
from gpu_common import lsq

pytestmark = pytest.mark.gpu

L = lsq._lib
FORCED = ("sliced 64 64", "sliced xmax 64", "window 96")


# ------------------------------------------------------------------------------------------------ helpers
def same_bits(a, b):
    """Equal as IEEE values including the sign of zero; NaN matches NaN (its payload is not part of any contract)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return bool(np.array_equal(a[ok].view(np.int64), b[ok].view(np.int64)))


def with_env(monkeypatch, env, fn):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return fn()
    finally:
        for k in env:
            monkeypatch.delenv(k, raising=False)


class Shape:
    """A handle kind with a pattern: host container around a value array, and the row of every stored value."""

    def __init__(self, name, kind, pattern, block=None, env=None, expect=None):
        self.name, self.kind, self.P, self.block, self.env, self.expect = name, kind, pattern, block, dict(env or {}), expect
        self.m, self.n = pattern.shape
        self.rows = pattern.indices.astype(np.int64)

    def host(self, V):
        if self.kind == "dense":
            return np.asfortranarray(V.reshape((self.m, self.n), order="F"))
        if self.kind == "block":
            return lsq.BlockDiagonal(*self.block, data=V.copy())
        if self.kind == "bordered":
            return lsq.BorderedBlockDiagonal(*self.block, data=V.copy())
        return sp.csc_matrix((V.copy(), self.P.indices, self.P.indptr), shape=self.P.shape)

    def device(self, ctx, monkeypatch, V):
        J = with_env(monkeypatch, self.env, lambda: lsq.DeviceMatrix(ctx, self.host(V)))
        if self.expect is not None:
            assert H.layout_matches(J.layout(), self.expect) == [], (self.name, J.layout())
        return J


def tall_column_pattern():
    """A column of 3000 entries beside columns of one."""
    m, n = 3000, 5
    rows = np.concatenate([[7], [2999], np.arange(m), [0], [1500]])
    indptr = np.array([0, 1, 2, 2 + m, 3 + m, 4 + m])
    return sp.csc_matrix((np.ones(rows.size), rows, indptr), shape=(m, n))


def _shapes():
    S = [Shape("dense %dx%d" % mn, "dense", H.full_pattern(*mn)) for mn in ((1, 1), (5, 1), (1, 6), (67, 33), (257, 3))]
    S += [Shape("csc %dx%d" % mn, "csc", H.full_pattern(*mn)) for mn in ((1, 1), (5, 1), (1, 6))]
    S.append(Shape("csc ragged", "csc", ac.ragged_pattern(300, 40, 0.08, 5)))
    S.append(Shape("csc tall column", "csc", tall_column_pattern()))
    for name in FORCED:
        cfg = H.CONFIGS[name]
        S.append(Shape("csc " + name, "csc", cfg.pattern, env=cfg.env, expect=cfg.expect))
    S += [Shape("block %s" % (b,), "block", H.block_pattern(*b), block=b) for b in ((7, 5, 3), (67, 33, 17))]
    S += [Shape("bordered %s" % (b,), "bordered", H.block_pattern(*b), block=b) for b in ((5, 8, 3, 2), (67, 33, 16, 5))]
    return {s.name: s for s in S}


SHAPES = _shapes()
READER_SHAPES = ["dense 67x33", "csc ragged", "csc tall column"] + ["csc " + n for n in FORCED] + \
    ["block (67, 33, 17)", "bordered (67, 33, 16, 5)"]


def values_and_factors(shape, seed, special=True, nan=True):
    rng = np.random.default_rng(seed)
    V = rng.uniform(0.5, 1.5, shape.rows.size) * rng.choice([-1.0, 1.0], shape.rows.size)
    w = H.factors(rng, shape.m)
    if special:
        sp_w = [0.0, -1.0, 2.0 ** -600] + ([np.nan] if nan else [])
        pos = rng.choice(shape.m, size=min(len(sp_w), shape.m), replace=False)
        w[pos] = sp_w[:pos.size]
    return V, w


def read_all(ctx, shape, J, vec, solve=True):
    """values, both products, both sums and one LSMR solve."""
    x, y, damp = vec
    out = [J.values(),
           lsq.mul_(lsq.DeviceVector(ctx, shape.m), J, lsq.DeviceVector(ctx, shape.n, x)).get(),
           lsq.mul_(lsq.DeviceVector(ctx, shape.n), J, lsq.DeviceVector(ctx, shape.m, y), trans=True).get(),
           lsq.colsumabs2_(lsq.DeviceVector(ctx, shape.n), J).get(),
           lsq.rowsumabs2_(lsq.DeviceVector(ctx, shape.m), J).get()]
    if solve:
        sv = lsq.AllocatedSolver(J, lsq.LSMR(), for_lm=True)
        xs, nmul = sv.ldiv_(lsq.DeviceVector(ctx, shape.n), lsq.DeviceVector(ctx, shape.m, y), lsq.DeviceVector(ctx, shape.n, damp))
        out += [xs.get(), np.array([float(nmul)])]
        sv.free()
    return out


def reader_vectors(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape.n), rng.standard_normal(shape.m), rng.uniform(0.05, 1.05, shape.n)


def assert_reads_like_fresh(ctx, monkeypatch, shape, J, expected, label):
    vec = reader_vectors(shape, 99)
    got = read_all(ctx, shape, J, vec)
    F = shape.device(ctx, monkeypatch, expected)
    try:
        want = read_all(ctx, shape, F, vec)
    finally:
        F.free()
    assert same_bits(got[0], expected), (label, "values")
    for k, (g, w) in enumerate(zip(got, want)):
        assert same_bits(g, w), (label, "reader %d differs from a fresh handle" % k)


# ------------------------------------------------------------------------------------------------ lsq_mat_scale_rows
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_scale_rows_bits(ctx, monkeypatch, name):
    shape = SHAPES[name]
    V, w = values_and_factors(shape, 11)
    J = shape.device(ctx, monkeypatch, V)
    try:
        J.scale_rows(w)
        assert same_bits(J.values(), V * w[shape.rows]), name
        J.scale_rows(lsq.DeviceVector(ctx, shape.m, np.full(shape.m, 2.0)))        # a DeviceVector, and a second pass
        assert same_bits(J.values(), (V * w[shape.rows]) * 2.0), name
    finally:
        J.free()


@pytest.mark.parametrize("name", READER_SHAPES)
def test_every_reader_after_scale_rows(ctx, monkeypatch, name):
    shape = SHAPES[name]
    V, w = values_and_factors(shape, 12, nan=False)
    J = shape.device(ctx, monkeypatch, V)
    try:
        J.scale_rows(w)
        assert_reads_like_fresh(ctx, monkeypatch, shape, J, V * w[shape.rows], name)
    finally:
        J.free()


def linear_f(shape, B):
    Rm = sp.csc_matrix((B, shape.P.indices, shape.P.indptr), shape=shape.P.shape).tocsr()

    def f_(out, x):
        out[:] = Rm @ x
    return f_


def mutate(ctx, shape, J, route, V2, keep):
    if route == "set_values":
        J.set_values(V2)
    elif route == "async":
        pb = lsq.PinnedBuffer(ctx, V2.size)
        pb.array[:] = V2
        keep.append(pb)
        J.set_values_async(pb)                      # (no upload_wait: the scaling must wait for the copy on the device)
    elif route == "write_refresh":
        ptr = lsq.lib().lsq_mat_values(J.h)
        lsq.DeviceVector.borrow(ctx, V2.size, C.c_void_p(ptr)).set(V2)
        J.refresh()
    elif route == "fd":
        if shape.kind == "csc":
            J.set_fd_colouring()
        lsq.fd_jacobian_(J, np.random.default_rng(5).uniform(-1.0, 1.0, shape.n), linear_f(shape, V2))
    elif route == "unscale_plain":                  # set_colscale(None) on a handle that has no scale: a refresh, no value changes
        J.set_colscale(None)
    elif route == "unscale":                        # a scale set and removed again: the stored values are back in charge
        s = lsq.DeviceVector(ctx, shape.n, H.factors(np.random.default_rng(6), shape.n))
        keep.append(s)
        J.set_colscale(s)
        J.set_colscale(None)
    else:
        raise KeyError(route)


REPLACING = ("set_values", "async", "write_refresh", "fd")       # routes that rewrite every value; the others leave them alone


@pytest.mark.parametrize("route", REPLACING + ("unscale_plain", "unscale"))
@pytest.mark.parametrize("name", ["dense 67x33", "csc ragged", "csc sliced 64 64", "block (7, 5, 3)", "bordered (5, 8, 3, 2)"])
def test_scale_rows_between_other_mutations(ctx, monkeypatch, name, route):
    shape = SHAPES[name]
    V, w = values_and_factors(shape, 13, nan=False)
    V2 = values_and_factors(shape, 14)[0]
    keep = []
    for first in ("route", "scale"):
        J = shape.device(ctx, monkeypatch, V)
        try:
            if first == "route":
                mutate(ctx, shape, J, route, V2, keep)
                # (differences of a linear f: to rounding; take what it wrote)
                base = J.values() if route == "fd" else V2 if route in REPLACING else V
                J.scale_rows(w)
                expected = base * w[shape.rows]
            else:
                J.scale_rows(w)
                mutate(ctx, shape, J, route, V2, keep)
                expected = J.values() if route == "fd" else V2 if route in REPLACING else V * w[shape.rows]
                if route == "fd":
                    assert np.allclose(expected, V2, rtol=1e-6, atol=1e-9)            # nothing of the scaled values is left
            assert_reads_like_fresh(ctx, monkeypatch, shape, J, expected, "%s %s first=%s" % (name, route, first))
        finally:
            J.upload_wait()
            J.free()
    for pb in keep:
        pb.free()


# the built-in model's g! on a sliced handle that multiplies out (LSQ_NO_COLSCALE=1) writes the mirrors ONLY and leaves the
# CSC-ordered copy stale: the one state in which the lsq_ensure_csc at the head of lsq_mat_scale_rows has work to do
LAZY = H.CONFIGS["g:sliced nocolscale"]


class LazyModel:
    """A TanhProblem on LAZY's pattern and its handle as a DeviceMatrix (the problem owns the handle)."""

    def __init__(self, ctx, monkeypatch, A):
        P = LAZY.pattern
        m, n = P.shape
        self.pr = with_env(monkeypatch, {"LSQ_NO_COLSCALE": "1"}, lambda: lsq.synthetic.TanhProblem(
            m, n, sparse=True, ctx=ctx, inputs=(P.indptr.astype(np.int32), P.indices.astype(np.int32), A)))
        J = lsq.DeviceMatrix.__new__(lsq.DeviceMatrix)
        J.ctx, J.h, J.m, J.n, J.nnz, J.sparse, J.blockdiag, J.bordered = ctx, self.pr.J, m, n, A.size, True, None, None
        self.J = J
        assert H.layout_matches(J.layout(), LAZY.expect) == [], J.layout()

    def g(self, x):
        self.pr.x.set(x)
        assert lsq.lib().lsq_model_g()(self.pr.J, self.pr.x.ptr, self.pr.model) == 0

    def close(self):
        self.J.h = None
        self.pr.close()


@pytest.mark.parametrize("first", ["g", "scale"])
def test_scale_rows_meets_a_stale_csc_copy(ctx, monkeypatch, first):
    shape = Shape("lazy", "csc", LAZY.pattern, expect=LAZY.expect)
    A, w = values_and_factors(shape, 17, nan=False)
    rng = np.random.default_rng(18)
    x1, x2 = rng.uniform(-1.0, 1.0, shape.n), rng.uniform(-1.0, 1.0, shape.n)
    md, shadow = LazyModel(ctx, monkeypatch, A), LazyModel(ctx, monkeypatch, A)
    try:
        md.g(x1)                                     # (the handle's CSC copy now holds nothing of any g!)
        if first == "scale":
            md.J.scale_rows(w)
            assert md.J.layout()["csc_fresh"]
        md.g(x2)
        assert md.J.layout()["csc_fresh"] is False
        shadow.g(x2)
        after_g = shadow.J.values()                  # read from a second model: values() on md would repair the state under test
        np.testing.assert_allclose(after_g, A * (1.0 - np.tanh(x2) ** 2)[np.repeat(np.arange(shape.n), np.diff(shape.P.indptr))],
                                   rtol=4e-16 * 8, atol=0)
        if first == "g":
            md.J.scale_rows(w)                       # must bring the CSC copy up to date BEFORE it scales and declares it
            assert md.J.layout()["csc_fresh"]
            expected = after_g * w[shape.rows]
        else:
            expected = after_g                       # g! replaced every value: nothing of the factors is left
        assert_reads_like_fresh(ctx, monkeypatch, shape, md.J, expected, "lazy g!, first=" + first)
    finally:
        md.close()
        shadow.close()


@pytest.mark.parametrize("mode", ["serial", "jitter"])
@pytest.mark.parametrize("name", ["dense 257x3", "csc sliced xmax 64", "bordered (67, 33, 16, 5)"])
def test_scale_rows_debug_modes_same_bits(ctx, monkeypatch, name, mode):
    shape = SHAPES[name]
    V, w = values_and_factors(shape, 15, nan=False)
    vec = reader_vectors(shape, 98)
    outs = []
    for debug in (False, True):
        if debug:
            lsq.debug_set(launch_jitter_us=200 if mode == "jitter" else 0, serial=1 if mode == "serial" else 0)
        try:
            J = shape.device(ctx, monkeypatch, V)
            J.scale_rows(w)
            outs.append(read_all(ctx, shape, J, vec))
            J.free()
        finally:
            lsq.debug_set(launch_jitter_us=0, serial=0)
    assert all(same_bits(a, b) for a, b in zip(*outs))
    assert same_bits(outs[0][0], V * w[shape.rows])


def test_scale_rows_refusals_leave_the_handle_usable(ctx, monkeypatch):
    shape = SHAPES["csc ragged"]
    V, w = values_and_factors(shape, 16, special=False)
    J = shape.device(ctx, monkeypatch, V)
    dw = lsq.DeviceVector(ctx, shape.m, w)
    s = lsq.DeviceVector(ctx, shape.n, np.full(shape.n, 1.5))
    try:
        assert lsq.lib().lsq_mat_scale_rows(J.h, None) == L.EARG and b"null" in lsq.lib().lsq_last_error()
        assert lsq.lib().lsq_mat_scale_rows(None, dw.ptr) == L.EARG
        with pytest.raises(lsq.DimensionMismatch):
            J.scale_rows(np.ones(shape.m + 1))
        J.set_colscale(s)
        with pytest.raises(lsq.ArgumentError, match="column scale"):
            J.scale_rows(dw)
        J.set_colscale(None)
        op = lsq.DeviceOperator(ctx, shape.m, shape.n, lambda t, x, o: None, lambda o: None)
        assert lsq.lib().lsq_mat_scale_rows(op.h, dw.ptr) == L.EARG and b"operator" in lsq.lib().lsq_last_error()
        op.free()
        assert same_bits(J.values(), V)                                  # no refusal wrote anything
        J.scale_rows(dw)
        assert_reads_like_fresh(ctx, monkeypatch, shape, J, V * w[shape.rows], "after the refusals")
    finally:
        J.free()


# ------------------------------------------------------------------------------------------------ lsq_loss_eval
def eval_inputs(m, c, seed, finite=False):
    rng = np.random.default_rng(seed)
    f = 3.0 * c * rng.standard_normal(m) * 10.0 ** rng.uniform(-2.0, 1.0, m)
    sp_in = R.transform_inputs(c)
    if finite:
        sp_in = sp_in[np.isfinite(sp_in)]
    k = min(m, sp_in.size)
    f[:k] = sp_in[:k]
    return f, 10.0 ** rng.uniform(-1.5, 1.5, m)


def full_grid_plus_one(ctx):
    return ctx.num_cus * 16 * 256 + 1        # one row past a full grid of the launch (LSQ_NT = 256)


@pytest.mark.parametrize("loss", R.BITWISE)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 257, "grid+1"])
def test_loss_eval_has_the_twins_bits(ctx, loss, weighted, m):
    m = full_grid_plus_one(ctx) if m == "grid+1" else m
    c = 0.37
    f, sigma = eval_inputs(m, c, 21 + m % 7)
    sigma = sigma if weighted else None
    if not weighted and m >= 64:
        f[-4:] = R.extreme_inputs(c)
    rt, rowf = lsq.loss_transform(f, loss, c, sigma)
    lo = lsq.Loss(ctx, loss, c, m, sigma)
    df, d1, d2 = lsq.DeviceVector(ctx, m, f), lsq.DeviceVector(ctx, m), lsq.DeviceVector(ctx, m)
    try:
        lo.eval(df, d1, d2)                                   # out of place, both outputs
        assert same_bits(d1.get(), rt) and same_bits(d2.get(), rowf) and same_bits(df.get(), f)
        mark = np.full(m, 7.0)
        d1.set(mark)
        lo.eval(df, None, d2)                                 # row factors only
        assert same_bits(d1.get(), mark) and same_bits(d2.get(), rowf)
        d2.set(mark)
        lo.eval(df, d1, None)                                 # residual only
        assert same_bits(d1.get(), rt) and same_bits(d2.get(), mark)
        lo.eval(df, None, None)                               # nothing asked for: nothing written
        assert same_bits(df.get(), f)
        lo.eval(df, df, d2)                                   # in place
        assert same_bits(df.get(), rt) and same_bits(d2.get(), rowf)
    finally:
        lo.free()


@pytest.mark.parametrize("loss", R.LOSSES)
@pytest.mark.parametrize("m", [1, 65, 257, "grid+1"])
def test_loss_eval_statistics(ctx, loss, m):
    m = full_grid_plus_one(ctx) if m == "grid+1" else m
    c = 0.37
    f, sigma = eval_inputs(m, c, 31, finite=True)
    lo = lsq.Loss(ctx, loss, c, m, sigma)
    df, d1 = lsq.DeviceVector(ctx, m, f), lsq.DeviceVector(ctx, m)
    try:
        count = int(np.sum(np.abs(f / sigma) / c > 1.0))
        ssr, out = lo.eval(df, d1, None, stats=True)
        assert ssr == lsq.sumsq(d1) and out == count
        ssr2, out2 = lo.eval(df, None, None, stats=True)      # no output buffer: the object's own scratch carries r~
        assert (ssr2, out2) == (ssr, out) and same_bits(df.get(), f)
        rt, rowf, ssr3, out3 = lo.transform(f)
        assert same_bits(rt, d1.get()) and (ssr3, out3) == (ssr, out)
    finally:
        lo.free()


@pytest.mark.parametrize("weighted", [False, True])
def test_cauchy_holds_the_accuracy_rule(ctx, weighted):
    c = 0.37
    f = np.concatenate([R.transform_inputs(c), R.grid_inputs(c)] + ([] if weighted else [R.extreme_inputs(c)]))
    sigma = 10.0 ** np.random.default_rng(7).uniform(-1.5, 1.5, f.size) if weighted else None
    lo = lsq.Loss(ctx, "cauchy", c, f.size, sigma)
    try:
        rt, rowf, _, _ = lo.transform(f)
    finally:
        lo.free()
    e_dev = R.transform_errors(rt, rowf, f, "cauchy", c, sigma)
    e_ref = R.transform_errors(*lsq.loss_transform(f, "cauchy", c, sigma), f, "cauchy", c, sigma)
    print("ROBUST cauchy sigma=%s | device e_rt %.3e e_w %.3e | twin e_rt %.3e e_w %.3e" % (weighted, e_dev[0], e_dev[1], e_ref[0], e_ref[1]))
    assert e_dev[0] <= ac.bound(e_ref[0], 1) and e_dev[1] <= ac.bound(e_ref[1], 1)
    assert R.nonfinite_classes_kept(rt, f)
    fin = np.isfinite(f)
    z = f if sigma is None else f / sigma
    assert np.all(np.abs(rt[fin]) <= np.abs(z[fin])) and np.array_equal(np.signbit(rt[fin]), np.signbit(z[fin]))
    w = rowf if sigma is None else rowf * sigma
    assert np.all((w >= 0.0) & (w <= 1.0 + (4e-16 if weighted else 0.0)))       # (times sigma again: one more rounding)


def test_loss_create_refusals(ctx):
    with pytest.raises(lsq.ArgumentError, match="unknown loss kind"):
        lsq.Loss(ctx, "tukey", 1.0, 4)
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(lsq.ArgumentError, match="finite and positive"):
            lsq.Loss(ctx, "huber", bad, 4)
        with pytest.raises(lsq.ArgumentError, match="entry 2"):
            lsq.Loss(ctx, "huber", 1.0, 4, np.array([1.0, 2.0, bad, 1.0]))
    with pytest.raises(lsq.DimensionMismatch):
        lsq.Loss(ctx, "huber", 1.0, 0)
    h = C.c_void_p()
    assert lsq.lib().lsq_loss_create(None, 1, 1.0, 4, None, C.byref(h)) == L.EARG
    assert lsq.lib().lsq_loss_create(ctx.h, 1, 1.0, 4, None, None) == L.EARG
    assert lsq.lib().lsq_loss_eval(None, None, None, None, None) == L.EARG
    assert lsq.lib().lsq_loss_destroy(None) == L.OK
    lo = lsq.Loss(ctx, "huber", 1.0, 4)                         # ... and the context still makes one
    assert lo.transform(np.array([0.5, -3.0, 0.0, 1.0]))[3] == 1
    lo.free()


# ------------------------------------------------------------------------------------------------ loops, bit for bit
RESULT_FIELDS = ("ssr", "iterations", "converged", "x_converged", "f_converged", "g_converged", "f_calls", "g_calls", "mul_calls")
C_SCALE = 2.0


def jacobian_values(J):
    return np.asarray(J).reshape(-1, order="F") if isinstance(J, np.ndarray) else J.data


def assert_same_fit(ra, rb, pa, pb, label):
    for k in RESULT_FIELDS:
        assert np.array_equal(getattr(ra, k), getattr(rb, k)), (label, k, getattr(ra, k), getattr(rb, k))
    assert same_bits(pa.x, pb.x), (label, "x")
    assert same_bits(pa.y, pb.y), (label, "y")
    assert same_bits(jacobian_values(pa.J), jacobian_values(pb.J)), (label, "J")
    assert (ra.trace is None) == (rb.trace is None)
    for k in (ra.trace or {}):
        assert same_bits(np.asarray(ra.trace[k], dtype=np.float64), np.asarray(rb.trace[k], dtype=np.float64)), (label, "trace", k)


def fit_pair(case, optimizer, loss, sigma, fd=False, run=lsq.optimize_, label="", **kw):
    """The loop with loss= on the raw problem, and the same loop on the robust_twin host problem."""
    pa = case.problem(g_=None if fd else "raw")
    pb = case.twin_problem(loss, C_SCALE, sigma, fd)
    ra = run(pa, optimizer, full_trace=True, loss=loss, f_scale=C_SCALE, sigma=sigma, **kw)
    rb = run(pb, optimizer, full_trace=True, **kw)
    assert_same_fit(ra, rb, pa, pb, "%s %s fd=%s %s" % (case.name, loss, fd, label))
    assert ra.loss == loss and ra.f_scale == C_SCALE and not hasattr(rb, "loss")
    return ra, pa


@pytest.mark.parametrize("loss", ["huber", "soft_l1", "linear"])
@pytest.mark.parametrize("solver", ["QR", "Cholesky"])
@pytest.mark.parametrize("optimizer", ["LevenbergMarquardt", "Dogleg"])
def test_decay_fits(ctx, optimizer, solver, loss):
    case = R.CASES["decay"]()
    ra, _ = fit_pair(case, getattr(lsq, optimizer)(getattr(lsq, solver)()), loss, case.sigma)
    assert ra.converged


LINE_ENVS = {"unsliced": {}, "sliced 64 64": H.CONFIGS["sliced 64 64"].env, "window 96": H.CONFIGS["window 96"].env}


@pytest.mark.parametrize("fd", [False, True])
@pytest.mark.parametrize("layout", sorted(LINE_ENVS))
@pytest.mark.parametrize("optimizer", ["LevenbergMarquardt", "Dogleg"])
def test_line_fits_over_lsmr(ctx, monkeypatch, optimizer, layout, fd):
    case = R.CASES["line"]()
    J = with_env(monkeypatch, LINE_ENVS[layout], lambda: lsq.DeviceMatrix(ctx, case.A))
    lay = J.layout()
    J.free()
    want = {"unsliced": (False, False, False), "sliced 64 64": (True, True, False), "window 96": (False, False, True)}[layout]
    assert (lay["srows"]["active"], lay["scols"]["active"], lay["nwin"] > 1) == want, lay      # the switches do what they say here
    with_env(monkeypatch, LINE_ENVS[layout],
             lambda: fit_pair(case, getattr(lsq, optimizer)(lsq.LSMR()), "huber", case.sigma, fd=fd, label=layout))


@pytest.mark.parametrize("fd", [False, True])
@pytest.mark.parametrize("solver", ["Cholesky", "BlockQR", "LSMR"])
def test_blocks_fits_as_one_problem(ctx, solver, fd):
    case = R.CASES["blocks"]()
    fit_pair(case, lsq.LevenbergMarquardt(getattr(lsq, solver)()), "huber", case.sigma, fd=fd)


def assert_same_batched(ra, rb, pa, pb, label):
    for k in ("ssr", "ssr0", "iterations", "converged", "x_converged", "f_converged", "g_converged", "f_calls", "g_calls", "mul_calls",
              "status", "info"):
        assert same_bits(np.asarray(getattr(ra, k), dtype=np.float64), np.asarray(getattr(rb, k), dtype=np.float64)), (label, k)
    assert ra.outer_iterations == rb.outer_iterations
    assert same_bits(pa.x, pb.x) and same_bits(pa.y, pb.y) and same_bits(pa.J.data, pb.J.data), label
    for k in ra.trace:
        assert same_bits(np.asarray(ra.trace[k], dtype=np.float64), np.asarray(rb.trace[k], dtype=np.float64)), (label, "trace", k)


@pytest.mark.parametrize("fd", [False, True])
@pytest.mark.parametrize("solver", ["Cholesky", "BlockQR"])
@pytest.mark.parametrize("optimizer", ["LevenbergMarquardt", "Dogleg"])
@pytest.mark.parametrize("size", ["B=1", "B=5", "300 copies"])
def test_blocks_fits_batched(ctx, size, optimizer, solver, fd):
    case = {"B=1": lambda: R.blocks_case(single=True), "B=5": R.blocks_case, "300 copies": lambda: R.blocks_case(copies=300)}[size]()
    opt = getattr(lsq, optimizer)(getattr(lsq, solver)())
    pa = case.problem(g_=None if fd else "raw")
    pb = case.twin_problem("soft_l1", C_SCALE, case.sigma, fd)
    ra = lsq.optimize_batched_(pa, opt, full_trace=True, iterations=60, loss="soft_l1", f_scale=C_SCALE, sigma=case.sigma)
    rb = lsq.optimize_batched_(pb, opt, full_trace=True, iterations=60)
    assert_same_batched(ra, rb, pa, pb, "%s %s %s fd=%s" % (size, optimizer, solver, fd))
    assert ra.loss == "soft_l1" and ra.outliers >= 0


@pytest.mark.parametrize("fd", [False, True])
@pytest.mark.parametrize("solver", ["Cholesky", "Schur", "BorderedQR", "LSMR"])
def test_global_fits(ctx, solver, fd):
    case = R.CASES["global"]()
    fit_pair(case, lsq.LevenbergMarquardt(getattr(lsq, solver)()), "huber", case.sigma, fd=fd)


def test_fit_with_bounds(ctx):
    case = R.CASES["decay"]()
    lower, upper = np.array([0.0, 0.0, -1.0]), np.array([4.5, 5.0, 0.3])     # the start is inside, the robust solution is not
    ra, pa = fit_pair(case, lsq.LevenbergMarquardt(lsq.QR()), "huber", case.sigma, lower=lower, upper=upper)
    assert np.all(pa.x >= lower) and np.all(pa.x <= upper) and (np.any(pa.x == lower) or np.any(pa.x == upper))


def test_allocated_problem_solved_twice(ctx):
    case = R.CASES["decay"]()
    opt = lsq.LevenbergMarquardt(lsq.Cholesky())
    na = lsq.LeastSquaresProblemAllocated(case.problem(), opt, ctx=ctx, loss="huber", f_scale=C_SCALE, sigma=case.sigma)
    nb = lsq.LeastSquaresProblemAllocated(case.twin_problem("huber", C_SCALE, case.sigma), opt, ctx=ctx)
    try:
        for start in (case.x0, case.x0 * 1.3 + 0.1):
            na.x[:] = start
            nb.x[:] = start
            ra, rb = lsq.optimize_(na, full_trace=True), lsq.optimize_(nb, full_trace=True)
            assert_same_fit(ra, rb, na, nb, "allocated")
            raw = np.zeros(case.m)
            case.f_(raw, na.x)
            assert ra.outliers == int(np.sum(np.abs(raw / case.sigma) / C_SCALE > 1.0)) >= 1
        with pytest.raises(TypeError):
            lsq.optimize_(na, loss="huber")
    finally:
        na.free()
        nb.free()


def raw_optimize(ctx, case, F, G, user, optimizer, solver):
    """lsq_optimize through ctypes on fresh device buffers: (status, result fields, x, y, values)."""
    Jd = lsq.DeviceMatrix(ctx, case.new_J())
    dx, dy = lsq.DeviceVector(ctx, case.n, case.x0), lsq.DeviceVector(ctx, case.m)
    try:
        st, res, tr = lsq.api._run_native(ctx, optimizer, solver, Jd, dx, dy, F, G, user, 1e-8, 1e-8, 1e-8, 200, None, (), (), True,
                                          case.n)
        return st, [getattr(res, k) for k in RESULT_FIELDS], dx.get(), dy.get(), Jd.values(), tr
    finally:
        Jd.free()


def host_f_callback(ctx, case, f_):
    xh, yh = np.zeros(case.n), np.zeros(case.m)

    def cb(d_out, d_x, _):
        L.check(lsq.lib().lsq_d2h(ctx.h, xh.ctypes.data_as(C.c_void_p), d_x, case.n * 8))
        f_(yh, xh)
        L.check(lsq.lib().lsq_h2d(ctx.h, d_out, yh.ctypes.data_as(C.c_void_p), case.m * 8))
        return 0
    return L.F_CALLBACK(cb)


@pytest.mark.parametrize("loss", ["huber", "soft_l1"])
@pytest.mark.parametrize("solver", ["QR", "CHOLESKY"])
@pytest.mark.parametrize("optimizer", ["LEVENBERG_MARQUARDT", "DOGLEG"])
def test_raw_lsq_optimize_with_device_differences(ctx, optimizer, solver, loss):
    """The C ABI as a C caller uses it, on the dense case with g = NULL (the Python layer differentiates a dense problem on the
    host): lsq_loss_f and a null g against the twin's f and a null g -- central differences of the wrapped residual on the
    device on both sides."""
    case = R.CASES["decay"]()
    opt, sol = getattr(L, optimizer), getattr(L, solver)
    lo = lsq.Loss(ctx, loss, C_SCALE, case.m, case.sigma)
    inner = host_f_callback(ctx, case, case.f_)
    twin = host_f_callback(ctx, case, lsq.robust_twin(case.f_, None, loss, C_SCALE, case.sigma)[0])
    try:
        lo.set_problem(inner, None)
        a = raw_optimize(ctx, case, lo.F, L.G_CALLBACK(), lo.h, opt, sol)
        b = raw_optimize(ctx, case, twin, L.G_CALLBACK(), None, opt, sol)
    finally:
        lo.free()
    assert a[0] == b[0] == L.OK and a[1] == b[1] and a[1][RESULT_FIELDS.index("converged")]
    assert all(same_bits(u, v) for u, v in zip(a[2:5], b[2:5]))
    assert all(same_bits(np.asarray(a[5][k], dtype=np.float64), np.asarray(b[5][k], dtype=np.float64)) for k in a[5])


@pytest.mark.parametrize("name,optimizer,solver", [("decay", "Dogleg", "QR"), ("line", "LevenbergMarquardt", "LSMR"),
                                                   ("global", "LevenbergMarquardt", "BorderedQR")])
def test_cauchy_wiring(ctx, name, optimizer, solver):
    """cauchy is not bitwise against numpy (log1p), so the comparator transforms ON THE DEVICE: host f_ / g_, then Loss.eval
    and DeviceMatrix.scale_rows by hand -- the bits of optimize_(loss="cauchy") by construction of the wrapper."""
    case = R.CASES[name]()
    opt = getattr(lsq, optimizer)(getattr(lsq, solver)())
    pa = case.problem()
    ra = lsq.optimize_(pa, opt, full_trace=True, loss="cauchy", f_scale=C_SCALE, sigma=case.sigma)
    lo = lsq.Loss(ctx, "cauchy", C_SCALE, case.m, case.sigma)
    raw, rowf = lsq.DeviceVector(ctx, case.m), lsq.DeviceVector(ctx, case.m)
    Jh = case.new_J()
    Jd = lsq.DeviceMatrix(ctx, Jh)
    xh, yh = np.zeros(case.n), np.zeros(case.m)

    def fcb(d_out, d_x, _):
        L.check(lsq.lib().lsq_d2h(ctx.h, xh.ctypes.data_as(C.c_void_p), d_x, case.n * 8))
        case.f_(yh, xh)
        out = lsq.DeviceVector.borrow(ctx, case.m, d_out)
        out.set(yh)
        lo.eval(out, out, None)
        return 0

    def gcb(_jh, d_x, _):
        L.check(lsq.lib().lsq_d2h(ctx.h, xh.ctypes.data_as(C.c_void_p), d_x, case.n * 8))
        case.g_(Jh, xh)
        Jd.set_values(jacobian_values(Jh))
        case.f_(yh, xh)
        raw.set(yh)
        lo.eval(raw, None, rowf)
        Jd.scale_rows(rowf)
        return 0

    dx, dy = lsq.DeviceVector(ctx, case.n, case.x0), lsq.DeviceVector(ctx, case.m)
    F, G = L.F_CALLBACK(fcb), L.G_CALLBACK(gcb)
    try:
        st, res, tr = lsq.api._run_native(ctx, opt.kind, opt.solver.kind, Jd, dx, dy, F, G, None, 1e-8, 1e-8, 1e-8, 1000, None, (),
                                          (), True, case.n)
        assert st == L.OK
        for k in RESULT_FIELDS:
            assert getattr(res, k) == getattr(ra, k), k
        assert same_bits(dx.get(), pa.x) and same_bits(dy.get(), pa.y) and same_bits(Jd.values(), jacobian_values(pa.J))
        for k in tr:
            assert same_bits(np.asarray(tr[k], dtype=np.float64), np.asarray(ra.trace[k], dtype=np.float64)), k
    finally:
        lo.free()
        Jd.free()


# ------------------------------------------------------------------------------------------------ limiting cases
@pytest.mark.parametrize("name,optimizer,solver", [("decay", "Dogleg", "QR"), ("line", "LevenbergMarquardt", "LSMR"),
                                                   ("blocks", "LevenbergMarquardt", "Cholesky")])
def test_huber_with_a_huge_scale_is_the_loop_without_a_loss(ctx, name, optimizer, solver):
    case = R.CASES[name]()
    opt = getattr(lsq, optimizer)(getattr(lsq, solver)())
    pa, pb = case.problem(), case.problem()
    ra = lsq.optimize_(pa, opt, full_trace=True, loss="huber", f_scale=1e300)
    rb = lsq.optimize_(pb, opt, full_trace=True)
    assert_same_fit(ra, rb, pa, pb, name)
    assert ra.outliers == 0


@pytest.mark.parametrize("name,optimizer,solver", [("decay", "Dogleg", "QR"), ("line", "LevenbergMarquardt", "LSMR"),
                                                   ("global", "LevenbergMarquardt", "Schur")])
def test_linear_with_sigmas_is_the_hand_weighted_problem(ctx, name, optimizer, solver):
    """Hand-weighted: f / sigma, and J times the ONE rounded factor 1 / sigma per row."""
    case = R.CASES[name]()
    opt = getattr(lsq, optimizer)(getattr(lsq, solver)())
    inv = 1.0 / case.sigma

    def hf(o, x):
        case.f_(o, x)
        o[:] = o / case.sigma

    def hg(J, x):
        case.g_(J, x)
        lsq.api._scale_rows_host(J, inv)

    pa, pb = case.problem(), case.problem(hf, hg)
    ra = lsq.optimize_(pa, opt, full_trace=True, sigma=case.sigma)
    rb = lsq.optimize_(pb, opt, full_trace=True)
    assert_same_fit(ra, rb, pa, pb, name)


@pytest.mark.parametrize("loss", ["huber", "soft_l1"])
@pytest.mark.parametrize("optimizer", ["LevenbergMarquardt", "Dogleg"])
def test_line_reaches_the_minimiser_of_the_convex_cost(ctx, optimizer, loss):
    case = R.CASES["line"]()
    g_tol = R.gradient_tolerance(case, loss, C_SCALE, case.sigma)
    p = case.problem()
    r = lsq.optimize_(p, getattr(lsq, optimizer)(lsq.LSMR()), full_trace=True, x_tol=0.0, f_tol=0.0, g_tol=g_tol, loss=loss,
                      f_scale=C_SCALE, sigma=case.sigma)
    assert r.converged and r.g_converged
    grad, gmax, bound = R.robust_gradient(case, R.measured_point(r, case.x0), loss, C_SCALE, case.sigma)
    print("ROBUST line %s %s | %d iterations, g_tol %.3e, |grad|_inf %.3e, product bound %.3e, outliers %d"
          % (optimizer, loss, r.iterations, g_tol, gmax, float(np.max(bound)), r.outliers))
    assert np.all(np.abs(grad) <= g_tol + bound)
    assert abs(gmax - r.trace["gnorm"][-1]) <= float(np.max(bound))
    assert R.robust_gradient(case, p.x, loss, C_SCALE, case.sigma)[1] <= R.LAST_STEP_FACTOR * g_tol     # ... and at the x the user gets
    raw = np.zeros(case.m)
    case.f_(raw, p.x)
    rho = R.reference(raw, loss, C_SCALE, case.sigma)[2]
    assert abs(r.ssr - float(C_SCALE ** 2 * np.sum(rho))) <= 1e-12 * r.ssr
    if loss == "huber":
        assert r.outliers == case.outliers.size == 30


# ------------------------------------------------------------------------------------------------ covariance on the live handle
@pytest.mark.parametrize("displaced", [True, False])
def test_bordered_qr_covariance_after_a_weighted_fit(ctx, displaced):
    case = R.global_case(displaced)
    opt = lsq.LevenbergMarquardt(lsq.BorderedQR())
    na = lsq.LeastSquaresProblemAllocated(case.problem(), opt, ctx=ctx, sigma=case.sigma)
    try:
        r = lsq.optimize_(na)
        assert r.converged
        sv = lsq.AllocatedSolver(na._Jd, lsq.BorderedQR(), for_lm=True)
        live = sv.bordered_qr_covariance(f=na._dy, cross=True)
        sv.free()
        B, mb, nb, ng = na._Jd.bordered
        Jf = lsq.DeviceMatrix(ctx, lsq.BorderedBlockDiagonal(B, mb, nb, ng, data=na.J.data.copy()))    # J~, as optimize_ left it
        sf = lsq.AllocatedSolver(Jf, lsq.BorderedQR(), for_lm=True)
        fresh = sf.bordered_qr_covariance(f=na.y, cross=True)                                          # r~
        sf.free()
        Jf.free()
        for k in ("cov", "stderr", "cross"):
            assert same_bits(getattr(live, k), getattr(fresh, k)), k
        if displaced:
            return
        # ... and on data without displaced rows (where the plain weighted fit stays well conditioned) it is the textbook
        # weighted covariance s^2 inv(J' W J), W = diag(1 / sigma^2): numpy on the J~ = diag(1 / sigma) J the fit left in nls.J
        # (the Jacobian of the last g!, one step before the returned x) and on r~, through a QR factor, to cond(J~) eps
        D = na.J.toarray()
        Rinv = np.linalg.inv(np.linalg.qr(D)[1])
        ref = np.sqrt(np.sum(Rinv ** 2, axis=1) * (na.y @ na.y) / (case.m - case.n))
        cond = np.linalg.cond(D)
        tol = 1e3 * cond * 2.0 ** -53
        print("ROBUST weighted covariance | cond %.2e, max rel diff of stderr %.2e, tol %.2e"
              % (cond, np.max(np.abs(live.stderr - ref) / ref), tol))
        assert cond < 1e7 and np.max(np.abs(live.stderr - ref) / ref) <= tol
    finally:
        na.free()


def test_dense_qr_covariance_after_a_robust_fit(ctx):
    case = R.CASES["decay"]()
    na = lsq.LeastSquaresProblemAllocated(case.problem(), lsq.Dogleg(lsq.QR()), ctx=ctx, loss="huber", f_scale=C_SCALE, sigma=case.sigma)
    try:
        assert lsq.optimize_(na).converged
        sv = lsq.AllocatedSolver(na._Jd, lsq.QR(), for_lm=False)
        live = sv.dense_qr_covariance(f=na._dy)
        sv.free()
        Jf = lsq.DeviceMatrix(ctx, na.J.copy())
        fresh = lsq.dense_qr_covariance(Jf, f=na.y)
        Jf.free()
        assert same_bits(live.cov, fresh.cov) and same_bits(live.stderr, fresh.stderr)
    finally:
        na.free()


# ------------------------------------------------------------------------------------------------ failures
class Boom(RuntimeError):
    pass


def test_inner_f_failing_inside_the_wrappers_g(ctx):
    case = R.CASES["decay"]()
    calls = {"n": 0, "fail_at": 2}          # call 1: the loop's f at x0; call 2: the evaluation inside lsq_loss_g

    def f_(o, x):
        calls["n"] += 1
        if calls["n"] == calls["fail_at"]:
            raise Boom("f_ fails")
        case.f_(o, x)

    opt = lsq.LevenbergMarquardt(lsq.QR())
    na = lsq.LeastSquaresProblemAllocated(case.problem(f_), opt, ctx=ctx, loss="huber", f_scale=C_SCALE, sigma=case.sigma)
    nb = lsq.LeastSquaresProblemAllocated(case.twin_problem("huber", C_SCALE, case.sigma), opt, ctx=ctx)
    try:
        with pytest.raises(Boom):
            lsq.optimize_(na)
        assert b"lsq_loss_g: the inner f callback reported failure" in lsq.lib().lsq_last_error()
        # the status a C caller sees
        calls.update(n=0, fail_at=2)
        dx, dy = lsq.DeviceVector(ctx, case.n, case.x0), lsq.DeviceVector(ctx, case.m)
        inner = host_f_callback(ctx, case, case.f_)

        def failing(d_out, d_x, _):
            calls["n"] += 1
            return 1 if calls["n"] == calls["fail_at"] else inner(d_out, d_x, None)

        lo = lsq.Loss(ctx, "huber", C_SCALE, case.m, case.sigma)
        lo.set_problem(L.F_CALLBACK(failing), L.G_CALLBACK(lambda j, x, u: 0))
        st, _, _ = lsq.api._run_native(ctx, opt.kind, opt.solver.kind, na._Jd, dx, dy, lo.F, lo.G, lo.h, 1e-8, 1e-8, 1e-8, 10, None,
                                       (), (), False, case.n)
        assert st == L.ECALLBACK and b"lsq_loss_g: the inner f callback reported failure" in lsq.lib().lsq_last_error()
        lo.free()
        # handle and loss object are usable: the next run is the twin's
        calls.update(n=0, fail_at=-1)
        na.x[:] = case.x0
        ra, rb = lsq.optimize_(na, full_trace=True), lsq.optimize_(nb, full_trace=True)
        assert_same_fit(ra, rb, na, nb, "after a failure")
    finally:
        na.free()
        nb.free()


def test_the_wrappers_reason_survives_the_loop_and_nothing_else(ctx):
    """lsq_last_error after LSQ_ECALLBACK: the wrapper's reason when the wrapper failed -- also when central differences report
    the failure first and the loop a second time --, and the loop's own text when somebody else's callback fails after a
    wrapper that failed outside any loop."""
    case = R.CASES["decay"]()
    opt, sol = L.LEVENBERG_MARQUARDT, L.QR
    Jd = lsq.DeviceMatrix(ctx, case.new_J())
    dx, dy = lsq.DeviceVector(ctx, case.n, case.x0), lsq.DeviceVector(ctx, case.m)
    inner = host_f_callback(ctx, case, case.f_)
    calls = {"n": 0}

    def second_call_fails(d_out, d_x, _):
        calls["n"] += 1
        return 1 if calls["n"] == 2 else inner(d_out, d_x, None)

    def run(F, G, user):
        st, _, _ = lsq.api._run_native(ctx, opt, sol, Jd, dx, dy, F, G, user, 1e-8, 1e-8, 1e-8, 5, None, (), (), False, case.n)
        return st, lsq.lib().lsq_last_error()

    lo = lsq.Loss(ctx, "huber", C_SCALE, case.m, case.sigma)
    try:
        # g = NULL: the second evaluation of f is the first one inside the central differences
        lo.set_problem(L.F_CALLBACK(second_call_fails), None)
        st, msg = run(lo.F, L.G_CALLBACK(), lo.h)
        assert st == L.ECALLBACK and b"lsq_loss_f: the inner f callback reported failure" in msg, msg
        # a wrapper failing outside any loop leaves its reason ...
        short = lsq.DeviceMatrix(ctx, np.zeros((case.m - 1, 3)))
        lo.set_problem(inner, L.G_CALLBACK(lambda j, x, u: 0))
        assert lo.G(short.h, dx.ptr, lo.h) != 0 and b"rows" in lsq.lib().lsq_last_error()
        short.free()
        # ... which must not stand in for the failure of a plain user callback in the next loop
        st, msg = run(L.F_CALLBACK(lambda o, x, u: 1), L.G_CALLBACK(lambda j, x, u: 0), None)
        assert st == L.ECALLBACK and msg == b"user callback reported failure", msg
    finally:
        lo.free()
        Jd.free()


def test_nan_residual_is_reported_at_the_plain_loops_index(ctx):
    case = R.CASES["decay"]()

    def f_(o, x):
        case.f_(o, x)
        o[17] = np.nan
        o[29] = np.inf

    seen = []
    for kw in ({}, dict(loss="cauchy", f_scale=C_SCALE, sigma=case.sigma), dict(loss="huber", f_scale=C_SCALE)):
        with pytest.raises(lsq.IsFiniteException) as e:
            lsq.optimize_(case.problem(f_), lsq.Dogleg(lsq.QR()), **kw)
        seen.append(e.value.indices)
    assert seen[0] == seen[1] == seen[2]


def test_wrapper_refuses_what_scale_rows_refuses(ctx):
    case = R.CASES["line"]()
    A = case.A

    def mul(t, x, out):
        raise AssertionError("never reached")

    op = lsq.DeviceOperator(ctx, case.m, case.n, mul, lambda o: None)
    p = lsq.LeastSquaresProblem(x=case.x0.copy(), y=np.zeros(case.m), f_=case.f_, g_=lambda J, x: None, J=op)
    with pytest.raises(lsq.LsqError, match="matrix-free operator") as e:
        lsq.optimize_(p, lsq.LevenbergMarquardt(lsq.LSMR()), loss="huber")
    assert e.value.status == L.ECALLBACK
    op.free()
    # a column-scaled handle, through the callback itself
    Jd = lsq.DeviceMatrix(ctx, A)
    s = lsq.DeviceVector(ctx, case.n, np.full(case.n, 0.5))
    Jd.set_colscale(s)
    lo = lsq.Loss(ctx, "huber", C_SCALE, case.m)
    dx = lsq.DeviceVector(ctx, case.n, case.x0)
    try:
        assert lo.G(Jd.h, dx.ptr, lo.h) != 0 and b"no problem behind the loss" in lsq.lib().lsq_last_error()
        lo.set_problem(host_f_callback(ctx, case, case.f_), L.G_CALLBACK(lambda j, x, u: 0))
        assert lo.G(Jd.h, dx.ptr, lo.h) != 0 and b"column scale" in lsq.lib().lsq_last_error()
        short = lsq.DeviceMatrix(ctx, np.zeros((case.m - 1, 3)))
        assert lo.G(short.h, dx.ptr, lo.h) != 0 and b"rows" in lsq.lib().lsq_last_error()
        short.free()
        Jd.set_colscale(None)
        before = Jd.values()
        assert lo.G(Jd.h, dx.ptr, lo.h) == 0                               # usable afterwards: g (a no-op here), then the scaling
        raw = np.zeros(case.m)
        case.f_(raw, case.x0)
        assert same_bits(Jd.values(), before * lsq.loss_transform(raw, "huber", C_SCALE)[1][A.indices])
    finally:
        lo.free()
        Jd.free()
