"""LSMR(): every stopping rule and breakdown that the reference reaches at the fixed tolerances, on every iteration driver of the
library.  The cases and their certified (iter, istop), margins and e_ref come from tests/lsmr_cases.py, certified without a
device by tests/test_lsmr_stops_host.py; x_hp is the longdouble twin (tests/lsmr_reference.py) at the same iteration count.

Drivers -- which copy of the seven rules decides, and how the test KNOWS it ran (info()["lsmr_path"], lsq_solver_lsmr_path:
no other accessor says which iteration ran; the layouts a handle built are DeviceMatrix.layout(), lsq_mat_layout):
    csc               unsliced CSC handle                                   lsmr_commit (k_lsmr_update)      "four-launch"
    sliced_four       LSQ_SELL_FORCE=1 handle, LSQ_LSMR_FOUR_LAUNCHES=1     lsmr_commit                      "four-launch"
                      (that the handle IS sliced: the same handle without the switch answers "three-launch", which
                      lsq_lsmr_solve takes only with both sliced layouts active and one column window)
    sliced_fused      LSQ_SELL_FORCE=1 handle                               lsmr_decide (k_lsmr_fused)       "three-launch"
    dense             dense handle                                          lsmr_commit                      "four-launch"
    general_p         LSMR(update, P) with P.ldiv = the default Jacobi      the host loop of lsq_lsmr_general.hip   "general"
    custom_p          LSMR(fn), fn restating the default Jacobi rule        lsmr_commit, custom_p setup      "four-launch"
    colscale          J = V diag(s), s powers of two, multiplied out        lsmr_commit                      "four-launch"
    colscale_sliced   the same on a sliced handle: s applied in the products   lsmr_decide                   "three-launch"
    operator          DeviceOperator over the same matrix                   lsmr_commit behind callbacks     "four-launch"
    reference_order   lsq.set_exact(True): the small-problem kernel         the loop of lsq_exact.hip        "reference-order"
The toy shapes (down to 3 x 2) do select the three-launch iteration under LSQ_SELL_FORCE=1 -- nothing in its conditions asks
for a size -- so no case is padded.

Per (case, driver): istop, iter, nmul as certified; damp <- sqrt(damp); y untouched; x finite; x == 0 exactly where x_hp == 0;
otherwise e_dev <= 16 max(e_ref, min(max(16, n), 64) 2^-53 iter) (ac.lsmr_bound), e_dev and e_ref both against x_hp in
||x - x_hp|| / ||x_hp||; the same solve again and under lsq.debug_set(serial=1): identical bits and counts.  Per driver: the
reuse sequence LC.REUSE on ONE solver (stops at iteration 0, 1, 2, 3, maxiter = 6, 0) against fresh solvers, bit for bit --
the double-buffer parity, the `done` flag and the epoch of the three-launch iteration.

Not here: the CAUTIOUS launch of k_lsmr_fused is asked for only by a trust-region loop that has a tail to place
(lsmr_run_fused: W.spec), never by a bare ldiv!; the trajectory tests of test_a_gpu_contract.py run it.  istop = 99 (a
hand-off that gives up) and row-sharded solves: tests/test_zz_gpu_stress.py, tests/test_rowshard.py."""
import numpy as np
import pytest
import scipy.sparse as sp

import accuracy_common as ac
import lsmr_cases as LC
from gpu_common import lsq

pytestmark = pytest.mark.gpu

DRIVERS = {"csc": "four-launch", "sliced_four": "four-launch", "sliced_fused": "three-launch", "dense": "four-launch",
           "general_p": "general", "custom_p": "four-launch", "colscale": "four-launch", "colscale_sliced": "three-launch",
           "operator": "four-launch", "reference_order": "reference-order"}
NAMES = list(LC.cases())


def _jacobi(cs, damp):
    if damp is not None:
        cs = cs + damp
    return np.where(cs > 0, 1.0 / np.sqrt(np.where(cs > 0, cs, 1.0)), 0.0)


class Driver:
    """One operand on one driver: the handle(s), a factory for solvers on it and the switches its solves run under."""

    def __init__(self, ctx, name, J, monkeypatch):
        self.ctx, self.name, self.mp = ctx, name, monkeypatch
        self.m, self.n = J.shape
        self.keep = []
        S = sp.csc_matrix(J)
        S.sort_indices()
        sliced = name in ("sliced_four", "sliced_fused", "colscale_sliced")
        if sliced:
            monkeypatch.setenv("LSQ_SELL_FORCE", "1")
        try:
            if name == "dense":
                self.J = lsq.DeviceMatrix(ctx, J)
            elif name in ("colscale", "colscale_sliced"):
                s = 2.0 ** ((np.arange(self.n) % 7) - 3.0)
                V = sp.csc_matrix((S.data / np.repeat(s, np.diff(S.indptr)), S.indices, S.indptr), shape=S.shape)
                assert np.array_equal(V.data * np.repeat(s, np.diff(S.indptr)), S.data)      # the effective operand, bit for bit
                self.J = lsq.DeviceMatrix(ctx, V)
                ds = lsq.DeviceVector(ctx, self.n, s)
                self.keep.append(ds)
                self.J.set_colscale(ds)
            elif name == "operator":
                inner = lsq.DeviceMatrix(ctx, S)
                self.keep.append(inner)
                self.J = lsq.DeviceOperator(ctx, self.m, self.n,
                                            lambda trans, x, out: lsq.mul_(out, inner, x, 1.0, 0.0, trans=trans),
                                            lambda out: lsq.colsumabs2_(out, inner))
            else:
                self.J = lsq.DeviceMatrix(ctx, S)
        finally:
            if sliced:
                monkeypatch.delenv("LSQ_SELL_FORCE")

    def solver(self, damped):
        ctx, n = self.ctx, self.n
        if self.name == "custom_p":
            def fn(P, Jm, dmp):
                P.set(_jacobi(lsq.colsumabs2_(lsq.DeviceVector(ctx, n), Jm).get(), None if dmp is None else dmp.get()))
            return lsq.AllocatedSolver(self.J, lsq.LSMR(fn), for_lm=damped)
        if self.name == "general_p":
            class JacobiP:
                d = np.ones(n)

                def ldiv(self, out, x):
                    out.set(x.get() * self.d)

            def update(Pobj, Jm, dmp):
                Pobj.d = _jacobi(lsq.colsumabs2_(lsq.DeviceVector(ctx, n), Jm).get(), None if dmp is None else dmp.get())
            return lsq.AllocatedSolver(self.J, lsq.LSMR(update, JacobiP()), for_lm=damped)
        return lsq.AllocatedSolver(self.J, lsq.LSMR(), for_lm=damped)

    def solve(self, sv, y, damp, four=None):
        four = self.name == "sliced_four" if four is None else four
        dy, dx = lsq.DeviceVector(self.ctx, self.m, y), lsq.DeviceVector(self.ctx, self.n, np.full(self.n, np.nan))
        dd = None if damp is None else lsq.DeviceVector(self.ctx, self.n, damp)
        if four:
            self.mp.setenv("LSQ_LSMR_FOUR_LAUNCHES", "1")
        try:
            _, nmul = sv.ldiv_(dx, dy) if dd is None else sv.ldiv_(dx, dy, dd)
        finally:
            if four:
                self.mp.delenv("LSQ_LSMR_FOUR_LAUNCHES")
        info = sv.info()
        return dict(x=dx.get(), nmul=nmul, istop=info["lsmr_istop"], iter=info["lsmr_iter"], path=info["lsmr_path"],
                    y=dy.get(), damp=None if dd is None else dd.get())


@pytest.fixture
def arithmetic(request):
    """Fast kernels for every driver but reference_order; the library's default again afterwards."""
    def choose(driver):
        lsq.set_exact(driver == "reference_order")
    yield choose
    lsq.set_exact(None)


def _counts(r):
    return r["nmul"], r["istop"], r["iter"], r["path"]


@pytest.mark.parametrize("driver", list(DRIVERS))
@pytest.mark.parametrize("name", NAMES)
def test_stop(ctx, name, driver, arithmetic, monkeypatch):
    z = LC.certify(name)
    c = z.case
    arithmetic(driver)
    D = Driver(ctx, driver, c.J, monkeypatch)
    prev = lsq.debug_get()
    try:
        lsq.debug_set(None, 0)
        r = D.solve(D.solver(c.damped), c.y, c.damp)
        again = D.solve(D.solver(c.damped), c.y, c.damp)
        lsq.debug_set(None, 1)
        serial = D.solve(D.solver(c.damped), c.y, c.damp)
        lsq.debug_set(None, 0)
        unforced = D.solve(D.solver(c.damped), c.y, c.damp, four=False) if driver == "sliced_four" else None
    finally:
        lsq.debug_set(prev[0], prev[1])
    e_dev = LC.rel_err(r["x"], z.x_hp)
    bound = ac.lsmr_bound(z.e_ref, c.n, z.iter)
    print("LSMRSTOP %-28s %-16s istop %d iter %d e_dev %.3e e_ref %.3e e_dev/bound %.3f"
          % (name, driver, r["istop"], r["iter"], e_dev, z.e_ref, e_dev / bound if bound > 0 else 0.0))
    # which copy of the rules ran
    assert r["path"] == DRIVERS[driver]
    if unforced is not None:
        assert unforced["path"] == "three-launch"
    # stop and counts
    assert (r["istop"], r["iter"], r["nmul"]) == (z.istop, z.iter, z.nmul)
    assert np.array_equal(r["y"], c.y)
    if c.damped:
        assert np.allclose(r["damp"], np.sqrt(c.damp), rtol=1e-15, atol=0.0)
    # finite, and as accurate as the tier asks
    assert np.all(np.isfinite(r["x"]))
    if not np.any(z.x_hp):
        assert not np.any(r["x"])
    else:
        assert e_dev <= bound, (e_dev, z.e_ref, bound)
    # repeatable, and independent of what was queued behind the deciding launch
    for other in (again, serial):
        assert _counts(other) == _counts(r)
        assert np.array_equal(other["x"], r["x"])


@pytest.mark.parametrize("driver", list(DRIVERS))
def test_reuse_of_one_solver(ctx, driver, arithmetic, monkeypatch):
    """LC.REUSE on ONE AllocatedSolver -- stops at iteration 0, 1, 2, 3, maxiter = 6 and 0 again -- against the same solves on
    fresh solvers: which buffer set holds the answer after an odd or an even stop, and what a finished solve leaves behind
    (`done`, the epoch, the hand-off record), must not reach the next solve."""
    seq = [LC.certify(n) for n in LC.REUSE]
    arithmetic(driver)
    D = Driver(ctx, driver, seq[0].case.J, monkeypatch)
    one = D.solver(False)
    for z in seq:
        r = D.solve(one, z.case.y, None)
        fresh = D.solve(D.solver(False), z.case.y, None)
        assert (r["istop"], r["iter"], r["nmul"], r["path"]) == (z.istop, z.iter, z.nmul, DRIVERS[driver]), z.case.name
        assert _counts(fresh) == _counts(r)
        assert np.array_equal(r["x"], fresh["x"]), z.case.name
