"""Handle state tier on the device: every reader after every mutation, on every layout (tests/handle_state_common.py has the
configurations, the twin, the committed sequences and oracle 2; tests/test_handle_state_host.py certifies them on the CPU).

Per configuration and committed sequence: the handle is built (its layout asserted through DeviceMatrix.layout()), then every
step applies one mutation and runs its readers, and each reader's output is held to two oracles:

  1. HISTORY INDEPENDENCE, bit for bit: np.array_equal the same reader on a FRESH handle of the same configuration that was
     given the twin's current V and s by set_values + set_colscale (a model handle whose scale is the model's: a fresh model
     handle and one g! at the same x).  No tolerance: the header's freshness contract promises the bits of a fresh handle.
  2. The twin's effective matrix through handle_state_common.judge (the bounds are stated there).

A g! that multiplies out (LSQ_NO_COLSCALE=1, segment / window / dense / block handles) and fd_jacobian_ produce values on the
device: they are held to A (1 - tanh(x)^2) at the rtol of test_device_g_values_stay_consistent, and to the linear model's
matrix within handle_state_common.fd_bound, and the twin then takes them over.  After such a g! they are read from a SHADOW
model handle that repeats every g!, never from the handle under test: values() would bring its CSC-ordered copy up to date and
with that undo the state the next mutation is meant to meet (layout()["csc_fresh"] is asserted False on the lazy
configuration).

The hand-written sequences at the end are the orderings the issue names.  Scale vectors and pinned buffers are kept alive by
the Bundle for the life of the handle; no pinned buffer is written after it was handed over."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import handle_state_common as H
from gpu_common import lsq
from oracle import oracle as O

pytestmark = pytest.mark.gpu

L = lsq._lib
G_RTOL = 4e-16 * 8                      # test_device_g_values_stay_consistent
CASES = [(name, k) for name in H.CONFIGS for k in range(H.NSEQ[name])]


@functools.lru_cache(maxsize=None)
def committed(name):
    return H.sequences(H.CONFIGS[name])


def host_matrix(cfg, twin, V):
    if cfg.kind == "dense":
        return np.asfortranarray(V.reshape(cfg.shape, order="F"))
    if cfg.kind == "block":
        return lsq.BlockDiagonal(*cfg.block, data=V)
    if cfg.kind == "bordered":
        return lsq.BorderedBlockDiagonal(*cfg.block, data=V)
    return sp.csc_matrix((V, twin.indices, twin.indptr), shape=cfg.shape)


class Bundle:
    """A handle with everything that must outlive it: the model (if any), scale vectors, pinned buffers, its solvers."""

    def __init__(self, ctx, cfg, twin):
        self.ctx, self.cfg, self.twin = ctx, cfg, twin
        self.J = self.pr = self.ds = None
        self.keep, self.solvers = [], {}
        self.vec = None

    def vectors(self):
        if self.vec is None:
            t, c = self.twin, self.ctx
            self.vec = dict(x=lsq.DeviceVector(c, t.n, t.x), y=lsq.DeviceVector(c, t.m, t.y))
        return self.vec

    def solver(self, name):
        if name not in self.solvers:
            kind = {"lsmr": lsq.LSMR, "cholesky": lsq.Cholesky, "qr": lsq.QR, "blockqr": lsq.BlockQR, "schur": lsq.Schur}[name]()
            self.solvers[name] = lsq.AllocatedSolver(self.J, kind, for_lm=True)
        return self.solvers[name]

    def close(self):
        for sv in self.solvers.values():
            sv.free()
        if self.pr is not None:
            self.J.h = None                 # (the problem owns the handle)
            self.pr.close()
        elif self.J is not None:
            self.J.free()
        for v in self.keep:
            v.free()


def with_env(monkeypatch, env, fn):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return fn()
    finally:
        for k in env:
            monkeypatch.delenv(k, raising=False)


def creation_env(cfg):
    return dict(cfg.env, **({"LSQ_NO_COLSCALE": "1"} if cfg.nocolscale else {}))


def plain_bundle(ctx, cfg, twin, V, monkeypatch):
    b = Bundle(ctx, cfg, twin)
    b.J = with_env(monkeypatch, cfg.env, lambda: lsq.DeviceMatrix(ctx, host_matrix(cfg, twin, V)))
    return b


def model_bundle(ctx, cfg, twin, A, monkeypatch):
    b = Bundle(ctx, cfg, twin)
    m, n = cfg.shape
    if cfg.kind == "block":
        make = lambda: lsq.synthetic.TanhProblem(m, n, ctx=ctx, inputs=A, blockdiag=cfg.block)       # noqa: E731
    elif cfg.kind == "dense":
        make = lambda: lsq.synthetic.TanhProblem(m, n, sparse=False, ctx=ctx, inputs=A)               # noqa: E731
    else:
        make = lambda: lsq.synthetic.TanhProblem(m, n, sparse=True, ctx=ctx,                          # noqa: E731
                                                 inputs=(twin.indptr.astype(np.int32), twin.indices.astype(np.int32), A))
    b.pr = with_env(monkeypatch, creation_env(cfg), make)
    J = lsq.DeviceMatrix.__new__(lsq.DeviceMatrix)
    J.ctx, J.h, J.m, J.n, J.nnz, J.sparse = ctx, b.pr.J, m, n, A.size, cfg.kind != "dense"
    J.blockdiag, J.bordered = (tuple(cfg.block) if cfg.kind == "block" else None), None
    b.J = J
    return b


def run_g(b, x):
    b.pr.x.set(x)
    assert lsq.lib().lsq_model_g()(b.pr.J, b.pr.x.ptr, b.pr.model) == 0


def set_scale(b, s, monkeypatch):
    ds = lsq.DeviceVector(b.ctx, b.twin.n, s)
    b.keep.append(ds)
    with_env(monkeypatch, {"LSQ_NO_COLSCALE": "1"} if b.cfg.nocolscale else {}, lambda: b.J.set_colscale(ds))
    b.ds = ds
    if b.cfg.scale_mode:
        assert b.J.layout()["colscale"] == b.cfg.scale_mode, (b.cfg.name, b.J.layout())


def assert_layout(b):
    lay = b.J.layout()
    assert H.layout_matches(lay, b.cfg.expect) == [], (b.cfg.name, lay)
    if b.cfg.kind == "block":
        assert b.J.blockdiag_info() == tuple(b.cfg.block)
    if b.cfg.kind == "bordered":
        assert b.J.bordered_info() == tuple(b.cfg.block)


class Shadow:
    """A second model handle that repeats every g! of the handle under test: where the values a g! produced are read."""

    def __init__(self, ctx, cfg, twin, monkeypatch):
        self.b = model_bundle(ctx, cfg, twin, twin.A, monkeypatch)

    def values_after_g(self, x, want):
        run_g(self.b, x)
        got = self.b.J.values()
        np.testing.assert_allclose(got, want, rtol=G_RTOL, atol=0)
        return got


def build(ctx, cfg, twin, monkeypatch):
    """The handle under test in the twin's initial state (+ the shadow of a model that multiplies out)."""
    if not cfg.model:
        b = plain_bundle(ctx, cfg, twin, twin.V, monkeypatch)
        if cfg.kind == "csc" and cfg.fd:
            assert b.J.set_fd_colouring() >= 1
        assert_layout(b)
        return b, None
    b = model_bundle(ctx, cfg, twin, twin.A, monkeypatch)
    assert_layout(b)
    run_g(b, twin.x_g)
    shadow = None
    if cfg.fused:
        assert b.J.layout()["colscale"] == "fused"
    else:
        assert b.J.layout()["colscale"] is None and b.J.layout()["csc_fresh"] == (not cfg.lazy), b.J.layout()
        shadow = Shadow(ctx, cfg, twin, monkeypatch)
        twin.V = shadow.values_after_g(twin.x_g, twin.V)
    return b, shadow


def fresh(ctx, cfg, twin, monkeypatch):
    """A new handle of the configuration holding the twin's current V and s."""
    if cfg.model and cfg.fused:
        b = model_bundle(ctx, cfg, twin, twin.V, monkeypatch)
        if twin.s is None:
            b.J.set_colscale(None)
        else:
            run_g(b, twin.x_g)
        return b
    b = plain_bundle(ctx, cfg, twin, twin.V, monkeypatch)
    if twin.s is not None:
        set_scale(b, twin.s, monkeypatch)
    return b


def linear_f(twin, B):
    R = sp.csc_matrix((B, twin.indices, twin.indptr), shape=(twin.m, twin.n)).tocsr()

    def f_(out, x):
        out[:] = R @ x
    return f_


def apply(b, shadow, mu, payload, rng, monkeypatch):
    """One mutation on the device; the twin has taken it already (payload = what twin.mutate returned)."""
    J, twin, ctx = b.J, b.twin, b.ctx
    if mu == "set_values":
        J.set_values(payload)
    elif mu in ("async_wait", "async_nowait"):
        pb = lsq.PinnedBuffer(ctx, payload.size)
        pb.array[:] = payload
        b.keep.append(pb)
        J.set_values_async(pb)
        if mu == "async_wait":
            J.upload_wait()
    elif mu == "write_refresh":
        ptr = lsq.lib().lsq_mat_values(J.h)
        assert ptr
        lsq.DeviceVector.borrow(ctx, payload.size, C.c_void_p(ptr)).set(payload)
        J.refresh()
    elif mu in ("set_colscale", "set_colscale_again"):
        set_scale(b, payload, monkeypatch)
    elif mu == "s_inplace":
        b.ds.set(payload)
        J.colscale_changed()
    elif mu in ("unscale", "unscale_plain"):
        J.set_colscale(None)
        assert J.layout()["colscale"] is None
    elif mu == "fd":
        x = rng.uniform(-1.0, 1.0, twin.n)
        lsq.fd_jacobian_(J, x, linear_f(twin, payload))
        got = J.values()
        assert np.all(np.abs(got - payload) <= H.fd_bound(twin, payload, x)), np.max(np.abs(got - payload))
        twin.V = got
    elif mu == "fd_refused":
        with pytest.raises(lsq.ArgumentError):
            lsq.fd_jacobian_(J, rng.uniform(-1.0, 1.0, twin.n), linear_f(twin, twin.V))
    elif mu == "g":
        run_g(b, payload)
        lay = J.layout()
        if b.cfg.fused:
            assert lay["colscale"] == "fused" and lay["csc_fresh"]
        else:
            assert lay["csc_fresh"] == (not b.cfg.lazy), lay
    else:
        raise KeyError(mu)


def read(b, reader):
    J, t, ctx = b.J, b.twin, b.ctx
    v = b.vectors()
    if reader == "values":
        return (J.values(),)
    if reader == "mul":
        return tuple(lsq.mul_(lsq.DeviceVector(ctx, t.m, t.yadd), J, v["x"], a, be).get() for a, be in H.ALPHA_BETA)
    if reader == "mul_t":
        return tuple(lsq.mul_(lsq.DeviceVector(ctx, t.n, t.xadd), J, v["y"], a, be, trans=True).get() for a, be in H.ALPHA_BETA)
    if reader == "colsum":
        return (lsq.colsumabs2_(lsq.DeviceVector(ctx, t.n), J).get(),)
    if reader == "rowsum":
        return (lsq.rowsumabs2_(lsq.DeviceVector(ctx, t.m), J).get(),)
    if reader.startswith("ldiv:"):
        sv = b.solver(reader[5:])
        x, nmul = sv.ldiv_(lsq.DeviceVector(ctx, t.n), v["y"], lsq.DeviceVector(ctx, t.n, t.damp))    # (LSMR roots its damp)
        if reader == "ldiv:lsmr" and b.cfg.lsmr_path:
            assert sv.info()["lsmr_path"] == b.cfg.lsmr_path, (b.cfg.name, sv.info()["lsmr_path"])
        return (x.get(), nmul)
    if reader == "gram":
        return (lsq.sparse_gram(J),)
    if reader == "cov" and b.cfg.kind == "csc":
        sv = b.solver("lsmr")
        dcov, dse, info = lsq.DeviceVector(ctx, t.n * t.n), lsq.DeviceVector(ctx, t.n), np.zeros(1, dtype=np.int32)
        st = lsq.lib().lsq_sparse_covariance(sv.h, J.h, None, dcov.ptr, dse.ptr, info.ctypes.data_as(L.c_ip))
        if st == L.ENOTPD:                 # the documented refusal at a structurally empty column: a status, not a fault
            return ("ENOTPD", int(info[0]))
        L.check(st)
        return (dcov.get(), dse.get())
    if reader == "cov" and b.cfg.kind == "dense":
        c = b.solver("cholesky").dense_covariance()
        return (c.cov.reshape(-1, order="F"), c.stderr)
    if reader == "cov_qr":
        c = b.solver("qr").dense_qr_covariance()
        return (c.cov.reshape(-1, order="F"), c.stderr)
    if reader == "cov":
        c = b.solver("cholesky").covariance()
        return (c.cov, c.stderr)
    raise KeyError(reader)


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(u, w) if isinstance(u, np.ndarray) else u == w for u, w in zip(a, b))


def check_readers(ctx, cfg, b, outs, monkeypatch, label):
    """Both oracles for the outputs `outs` (reader -> what read() returned on the handle under test)."""
    twin = b.twin
    f = fresh(ctx, cfg, twin, monkeypatch)
    try:
        for reader, out in outs.items():
            assert same(out, read(f, reader)), (label, reader, "differs from a fresh handle")
            q = H.judge(twin, reader, out, O)
            print("STATE %s | %s | error / bound %.3g" % (label, reader, q))
            assert q <= 1.0, (label, reader, q)
    finally:
        f.close()


@pytest.mark.parametrize("name,k", CASES)
def test_committed_sequence(ctx, monkeypatch, name, k):
    cfg = H.CONFIGS[name]
    twin = H.Twin(cfg, H._seed(cfg, k))
    b, shadow = build(ctx, cfg, twin, monkeypatch)
    try:
        for i, (mu, readers) in enumerate(committed(name)[k]):
            rng = H.step_rng(cfg, k, i)
            payload = twin.mutate(mu, rng)
            apply(b, shadow, mu, payload, rng, monkeypatch)
            outs = {r: read(b, r) for r in readers}
            if mu == "g" and shadow is not None:
                twin.V = shadow.values_after_g(payload, twin.V)
            check_readers(ctx, cfg, b, outs, monkeypatch, "%s #%d step %d %s" % (name, k, i, mu))
    finally:
        b.close()
        if shadow is not None:
            shadow.b.close()


# ------------------------------------------------------------------------------------------------ hand-written orderings
LAZY = H.CONFIGS["g:sliced nocolscale"]
FEW = ("values", "mul", "mul_t", "colsum", "rowsum", "ldiv:lsmr", "gram")


def lazy_handle(ctx, cfg, monkeypatch, seed):
    """A model handle after two g! at different x, the CSC-ordered copy stale (asserted); the twin holds the values of the
    second one (from the shadow)."""
    twin = H.Twin(cfg, seed)
    b, shadow = build(ctx, cfg, twin, monkeypatch)
    x = twin.mutate("g", np.random.default_rng(seed + 1))
    run_g(b, x)
    assert b.J.layout()["csc_fresh"] is False and b.J.layout()["colscale"] is None
    twin.V = shadow.values_after_g(x, twin.V)
    shadow.b.close()
    return b, twin


@pytest.mark.parametrize("then", ["unscale_plain", "refresh", "set_colscale", "sparse_gram"])
def test_lazy_g_then(ctx, monkeypatch, then):
    """The stale CSC-ordered copy of a lazy g! met first by each of the entries that used to take it for current."""
    b, twin = lazy_handle(ctx, LAZY, monkeypatch, 41)
    try:
        outs = {}
        if then == "unscale_plain":
            b.J.set_colscale(None)
        elif then == "refresh":
            b.J.refresh()
        elif then == "set_colscale":
            twin.s = H.factors(np.random.default_rng(42), twin.n)
            set_scale(b, twin.s, monkeypatch)
        else:
            outs["gram"] = read(b, "gram")
        if then != "sparse_gram":
            assert b.J.layout()["csc_fresh"]
        outs.update({r: read(b, r) for r in FEW if r not in outs})
        check_readers(ctx, LAZY, b, outs, monkeypatch, "lazy g! then " + then)
    finally:
        b.close()


LAZY_BLOCK = H.Config("g:block lazy", "block", (140000, 11200), functools.lru_cache(maxsize=1)(lambda: H.block_pattern(1400, 100, 8)),
                      dict(kind="csc", srows=True, scols=True, ncw=1), None, model=True, nocolscale=True, lazy=True,
                      block=(1400, 100, 8))


def test_lazy_g_then_block_solve(ctx, monkeypatch):
    """The per-block Cholesky reads the CSC-ordered values: after a lazy g! on a block-diagonal handle large enough for the
    sliced layouts, its first solve."""
    b, twin = lazy_handle(ctx, LAZY_BLOCK, monkeypatch, 43)
    try:
        outs = {"ldiv:cholesky": read(b, "ldiv:cholesky")}
        f = plain_bundle(ctx, LAZY_BLOCK, twin, twin.V, monkeypatch)
        try:
            assert same(outs["ldiv:cholesky"], read(f, "ldiv:cholesky"))
        finally:
            f.close()
        B, mb, nb = LAZY_BLOCK.block
        E = twin.V.reshape(B, nb, mb)
        x = outs["ldiv:cholesky"][0].reshape(B, nb)
        for blk in range(0, B, 97):
            A = E[blk].T
            ref = np.linalg.lstsq(np.vstack([A, np.diag(np.sqrt(twin.damp[blk * nb:(blk + 1) * nb]))]),
                                  np.concatenate([twin.y[blk * mb:(blk + 1) * mb], np.zeros(nb)]), rcond=None)[0]
            assert np.max(np.abs(x[blk] - ref)) <= 1e-9 * np.max(np.abs(ref)), blk
    finally:
        b.close()


def test_lazy_g_then_batched_first_step(ctx, monkeypatch):
    """optimize_batched's first step (its kernels address the CSC-ordered values directly) on a problem whose handle was left
    with a stale CSC copy by g! at ANOTHER x: the same bits as on a new problem, and the step of a problem without sliced
    layouts (LSQ_NO_SELL=1: every g! writes the CSC-ordered copy) to the solve tolerance 1e-9."""
    cfg = LAZY_BLOCK
    twin = H.Twin(cfg, 44)
    x0 = np.random.default_rng(45).uniform(-0.5, 0.5, twin.n)
    res = []
    for stale, env in ((True, {}), (False, {}), (False, {"LSQ_NO_SELL": "1"})):
        b = with_env(monkeypatch, env, lambda: model_bundle(ctx, cfg, twin, twin.A, monkeypatch))
        try:
            if stale:
                run_g(b, twin.x_g)
                assert b.J.layout()["csc_fresh"] is False
            if env:
                assert not b.J.layout()["srows"]["active"]
            b.pr.reset(x0)
            r = b.pr.optimize_batched(iterations=1)
            res.append(r.minimizer.copy())
        finally:
            b.close()
    assert np.array_equal(res[0], res[1])
    assert np.max(np.abs(res[0] - x0)) > 1e-3                      # (a step was taken)
    assert np.max(np.abs(res[0] - res[2])) <= 1e-9 * np.max(np.abs(res[2]))


SEG = H.CONFIGS["segments"]


def test_async_uploads_on_two_handles_of_one_context(ctx, monkeypatch):
    """Both uploads record the context's one copy_done event; upload_wait on the FIRST handle only, then the second handle is
    read first."""
    twins = [H.Twin(SEG, 51), H.Twin(SEG, 52)]
    bs = [build(ctx, SEG, t, monkeypatch)[0] for t in twins]
    try:
        for b, t, seed in zip(bs, twins, (53, 54)):
            apply(b, None, "async_nowait", t.mutate("async_nowait", np.random.default_rng(seed)), None, monkeypatch)
        bs[0].J.upload_wait()
        for b in (bs[1], bs[0]):
            check_readers(ctx, SEG, b, {r: read(b, r) for r in FEW}, monkeypatch, "two async uploads")
    finally:
        for b in bs:
            b.close()


def test_async_upload_into_a_materialising_scale(ctx, monkeypatch):
    twin = H.Twin(SEG, 55)
    b, _ = build(ctx, SEG, twin, monkeypatch)
    try:
        rng = np.random.default_rng(56)
        apply(b, None, "set_colscale", twin.mutate("set_colscale", rng), rng, monkeypatch)
        assert b.J.layout()["colscale"] == "materialising"
        apply(b, None, "async_nowait", twin.mutate("async_nowait", rng), rng, monkeypatch)
        check_readers(ctx, SEG, b, {r: read(b, r) for r in FEW}, monkeypatch, "async upload under a multiplied-out scale")
    finally:
        b.close()


@pytest.mark.parametrize("name", ["segments", "sliced 64 64"])
def test_one_lsmr_solver_alternated_between_handles(ctx, monkeypatch, name):
    """The solver's column-sum cache is keyed on (handle uid, version): two handles of equal shape and equal version count but
    different values, one solver; one of them destroyed and a third created in between (possibly at its address)."""
    cfg = H.CONFIGS[name]
    twins = [H.Twin(cfg, 61 + i) for i in range(3)]
    b1, b2 = (build(ctx, cfg, t, monkeypatch)[0] for t in twins[:2])
    b3 = None
    sv = b1.solver("lsmr")

    def solve_on(b):
        sv.J = b.J
        b.solvers["lsmr"] = sv
        out = read(b, "ldiv:lsmr")
        del b.solvers["lsmr"]
        f = fresh(ctx, cfg, b.twin, monkeypatch)
        try:
            assert same(out, read(f, "ldiv:lsmr")), "differs from a fresh solver on a fresh handle"
        finally:
            f.close()
        assert H.judge(b.twin, "ldiv:lsmr", out, O) <= 1.0

    try:
        solve_on(b1)
        solve_on(b2)
        solve_on(b1)
        b2.close()
        b2 = None
        b3 = build(ctx, cfg, twins[2], monkeypatch)[0]
        solve_on(b3)
        solve_on(b1)
    finally:
        sv.J = b1.J
        b1.solvers["lsmr"] = sv
        for b in (b1, b2, b3):
            if b is not None:
                b.close()


@pytest.mark.parametrize("first", ["V", "s"])
def test_fused_colsum_after_values_and_scale_changed(ctx, monkeypatch, first):
    """The two version counters of the fused mode: colsumabs2(V) is cached on base_version, s.^2 .* it on version."""
    cfg = H.CONFIGS["sliced 64 64"]
    twin = H.Twin(cfg, 71)
    b, _ = build(ctx, cfg, twin, monkeypatch)
    try:
        rng = np.random.default_rng(72)
        apply(b, None, "set_colscale", twin.mutate("set_colscale", rng), rng, monkeypatch)
        assert b.J.layout()["colscale"] == "fused"
        read(b, "colsum")                                           # both caches are now current
        for mu in (("set_values", "s_inplace") if first == "V" else ("s_inplace", "set_values")):
            apply(b, None, mu, twin.mutate(mu, rng), rng, monkeypatch)
        check_readers(ctx, cfg, b, {r: read(b, r) for r in ("colsum", "ldiv:lsmr", "mul_t")}, monkeypatch, "V, s, colsum")
    finally:
        b.close()


def test_forced_sliced_rows_keep_the_sliced_kernels_in_default_mode(ctx, monkeypatch):
    """build_sliced_rows frees the CSR mirror the reference-order kernels read: a handle with sliced rows on a pattern small
    enough for them (only LSQ_SELL_FORCE builds one) is declined by lsq_small_mat and keeps the sliced kernels with
    reference-order mode ON, the default -- no set_exact(False) around it."""
    cfg = H.Config("small forced", "csc", (589, 129), H.CONFIGS["small"]._pattern, dict(kind="csc", srows=True, scols=True, ncw=1),
                   "fused", "three-launch", env={"LSQ_SELL_FORCE": "1", "LSQ_SELL_ROWS": "128", "LSQ_SELL_GROWS": "256"}, fd=False)
    twin = H.Twin(cfg, 81)
    b, _ = build(ctx, cfg, twin, monkeypatch)
    try:
        assert b.J.layout()["srows"]["wrows"] == 128
        check_readers(ctx, cfg, b, {r: read(b, r) for r in FEW}, monkeypatch, "small forced")
        rng = np.random.default_rng(82)
        apply(b, None, "set_colscale", twin.mutate("set_colscale", rng), rng, monkeypatch)
        check_readers(ctx, cfg, b, {r: read(b, r) for r in FEW}, monkeypatch, "small forced, scaled")
    finally:
        b.close()
