"""Trust-region tier: every LM / Dogleg branch and bound on every loop driver of the library.  The cases, their certified
counts, flags, accept patterns and branch-pure deltas come from tests/trust_region_cases.py, certified without a device by
tests/test_trust_region_host.py; the longdouble twin (tests/trust_region_reference.py) is the reference of every continuous
value.

Drivers -- which copy of the loop control / projected gradient / clip / clamp runs, and how the test KNOWS it did:
    dense_{qr,cholesky}_exact   dense handle, lsq.set_exact(True)       optimize_lm_loop / optimize_dogleg_loop with the
                                                                         reference-order kernels (lsq_exact_lm_damp, lsq_seq_reduce)
    dense_{qr,cholesky}_fast    dense handle, lsq.set_exact(False)      the same loops; k_lm_damp_grad / k_dl_scale, k_box_clip
    csc_lsmr                    CSC handle, LSMR(), fast kernels        k_lm_lsmr_setup (16 register slots of 1024 columns:
                                layout()["srows"]["active"] is False     n <= 16384) or, beyond, k_lm_damp + k_gradnorm; k_box_clip
    csc_lsmr_sliced             LSQ_SELL_FORCE=1: srows and scols active the same on the three-launch LSMR iteration
    csc_lsmr_separate           LSQ_LSMR_SEPARATE_SETUP=1               k_lm_damp_grad in front of the solve instead of
                                                                         k_lm_lsmr_setup (lsq_lsmr_takes_lm_prep reads the switch)
    model_sliced                synthetic.TanhProblem, LSQ_SELL_FORCE=1  built-in f! / g!; paths(): both sliced layouts, "three-launch"
                                                                         where x fits one column window (mat_layout: ncw == 1),
                                                                         "four-launch" from n = 16384 on.  Without bounds the tail is
                                                                         handed to the solve; with bounds tail_ok is false in
                                                                         optimize_lm_loop and the same tail runs unguarded behind
                                                                         k_box_clip (a condition of the code: no counter tells the two
                                                                         apart; pair_tails grows in both).  n = 16385 is past one
                                                                         workgroup: k_lm_damp + multi-block k_gradnorm
    sharded_world1              optimize_(row_allreduce=HostStaged...)   the sharded branch of optimize_lm_loop (LM + LSMR only)
    batched_{cholesky,blockqr}  optimize_batched_ on a BlockDiagonal     k_bt_step / k_bt_decide, the case as ONE block of
                                                                         B = 1, 5, 300 beside unrelated blocks
    operator_level              loops.optimize_operator_level            loops.py over the vector layer (k_reduce, k_box_clip, k_clamp)
    blockdiag_cholesky          BlockDiagonal through optimize_          optimize_*_loop; only the hand-over to the block solver is new
Scripted cases (Case.exact) run on the host-callback drivers; the index-spread cases (n = 1 ... 16385) on csc_lsmr*, and
model_sliced.

Per (case, driver): status, iterations, f_calls, g_calls, converged, the three flags and the accept pattern (LSMR drivers: the
inner counts too) EXACTLY as certified; every delta that is a pure function of its branch (halving, division by
decrease_factor or by 1/3, floor, cap, a tie that keeps it) bit for bit from the delta before it
(trust_region_reference.pure_delta); rho, ssr, gnorm, every delta and every x_k by
    e_dev <= 16 max(e_ref, floor)            (accuracy_common.trajectory_bound)
with e_dev / e_ref the device's and the float64 oracle's (same solver) distance from the longdouble twin at the same iteration
and the floor of a sum of max(m, n) terms per iteration so far, times ssr / pred_red for rho (and for a delta that LM computes
from rho: q > 1/3; no other delta) and max |J|'|f| / max |J'f| for gnorm, the condition numbers of those with respect to the
sums they are made of (trust_region_cases.trajectory_pieces, shared with the host tier's planted errors).  Where such a factor
exceeds COND_CAP = 1e6 the comparison is one of rounding errors: it is made, printed as such and left out of the worst ratio;
the host tier asserts how many there are;
every iterate of a bounded case inside its box; the same bits and counts on a second run and under lsq.debug_set(serial=1).
Refusals (x0 outside the bounds; a non-finite x) are compared as status codes.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import accuracy_common as ac
import trust_region_cases as TC
import trust_region_reference as R
from gpu_common import lsq
from oracle import oracle as O

pytestmark = pytest.mark.gpu

LD = np.longdouble
NAMES = list(TC.cases())
HOST_DRIVERS = ("dense_qr_exact", "dense_cholesky_exact", "dense_qr_fast", "dense_cholesky_fast", "csc_lsmr", "csc_lsmr_sliced",
                "csc_lsmr_separate", "sharded_world1", "operator_level", "blockdiag_cholesky")
ROWS = np.tile(np.arange(TC.M), TC.N)
COLPTR = np.arange(TC.N + 1) * TC.M
WORST = {}


def _solver_of(driver):
    if "lsmr" in driver or driver in ("sharded_world1", "operator_level"):
        return "lsmr", O.LSMR
    if "cholesky" in driver:
        return "direct", O.CHOLESKY
    return "direct", O.QR


_ORACLES = {}


def oracle_of(name, osolver):
    if (name, osolver) not in _ORACLES:
        _ORACLES[name, osolver] = TC.oracle(TC.cases()[name], osolver)
    return _ORACLES[name, osolver]


def _start_delta(case):
    d = case.opts["delta"]
    return d if d is not None else (10.0 if case.kind == "lm" else 1.0)


def _opts(case):
    o = dict(case.opts)
    o["lower"] = () if o["lower"] is None else o["lower"]
    o["upper"] = () if o["upper"] is None else o["upper"]
    return o


class Got:
    """What one run on the device left: status, the summary tuple of TC.summary, the trace."""

    def __init__(self, status, r=None):
        self.status, self.r = status, r
        self.trace = None if r is None else r.trace

    def summary(self):
        r = self.r
        if r is None:
            return (self.status,)
        return (self.status, int(r.iterations), bool(r.converged), bool(r.x_converged), bool(r.f_converged),
                bool(r.g_converged), int(r.f_calls), int(r.g_calls))

    def bits(self):
        if self.r is None:
            return self.summary()
        t = self.trace
        if t is None:
            return self.summary() + (np.asarray(self.r.minimizer).tobytes(), float(self.r.ssr))
        return self.summary() + tuple(np.asarray(t[k]).tobytes() for k in ("ssr", "gnorm", "delta", "rho", "accept", "x")) \
            + (np.asarray(self.r.minimizer).tobytes(),)


def _guard(fn):
    try:
        return Got(0, fn())
    except lsq._lib.LsqError as e:
        return Got(e.status)


def run_host_driver(ctx, case, driver, monkeypatch):
    """One toy case through optimize_ (or loops.py) on one driver."""
    p = case.make()
    m, n = case.m, case.n
    Opt = lsq.LevenbergMarquardt if case.kind == "lm" else lsq.Dogleg
    o = _opts(case)
    x, y = case.x0.copy(), np.zeros(m)
    if driver.startswith("dense"):
        nls = lsq.LeastSquaresProblem(x=x, y=y, f_=p.f, g_=p.g, J=np.zeros((m, n), order="F"))
        solver = lsq.QR() if "qr" in driver else lsq.Cholesky()
        return _guard(lambda: lsq.optimize_(nls, Opt(solver), full_trace=True, ctx=ctx, **o))
    if driver == "blockdiag_cholesky":
        def g_bd(J, xx):
            D = np.zeros((m, n))
            p.g(D, xx)
            J.data[:] = D.reshape(-1, order="F")
        nls = lsq.LeastSquaresProblem(x=x, y=y, f_=p.f, g_=g_bd, J=lsq.BlockDiagonal(1, m, n))
        return _guard(lambda: lsq.optimize_(nls, Opt(lsq.Cholesky()), full_trace=True, ctx=ctx, **o))

    def g_csc(J, xx):
        D = np.zeros((m, n))
        p.g(D, xx)
        J.data[:] = D.reshape(-1, order="F")

    S = sp.csc_matrix((np.ones(m * n), ROWS.copy(), COLPTR.copy()), shape=(m, n))
    nls = lsq.LeastSquaresProblem(x=x, y=y, f_=p.f, g_=g_csc, J=S)
    if driver == "operator_level":
        def run():
            r = lsq.loops.optimize_operator_level(nls, Opt(lsq.LSMR()), ctx=ctx,
                                                  **{k: v for k, v in o.items() if k != "delta" or v is not None})
            return r
        return _guard(run)
    if driver == "sharded_world1":
        from lsq_amd import rowshard as RS
        hook = RS.HostStagedRowAllreduce(ctx)
        return _guard(lambda: lsq.optimize_(nls, Opt(lsq.LSMR()), full_trace=True, ctx=ctx, row_allreduce=hook, global_rows=m, **o))
    sliced = driver == "csc_lsmr_sliced"
    if sliced:
        monkeypatch.setenv("LSQ_SELL_FORCE", "1")
    try:
        alloc = lsq.LeastSquaresProblemAllocated(nls, Opt(lsq.LSMR()), ctx=ctx)
    finally:
        if sliced:
            monkeypatch.delenv("LSQ_SELL_FORCE")
    lay = alloc._Jd.layout()
    assert lay["kind"] == "csc" and lay["srows"]["active"] == sliced and lay["scols"]["active"] == sliced, lay
    if driver == "csc_lsmr_separate":
        monkeypatch.setenv("LSQ_LSMR_SEPARATE_SETUP", "1")
    try:
        return _guard(lambda: lsq.optimize_(alloc, full_trace=True, **o))
    finally:
        if driver == "csc_lsmr_separate":
            monkeypatch.delenv("LSQ_LSMR_SEPARATE_SETUP")
        alloc.free()


def check_trajectory(label, driver, got, f64, ld, oracle, k, inner, start_delta, lower=None, upper=None, traced=True):
    """The assertions of the module docstring for one run against one certified case."""
    want = TC.summary(f64)
    assert TC.summary(oracle) == want, (label, "the oracle with this driver's solver is not the certified run")
    if f64.status != R.OK:
        assert got.status == f64.status, (label, got.status, f64.status)
        return
    assert got.summary() == want, (label, got.summary(), want)
    if not traced:          # (loops.py returns no trace: the end point stands for the trajectory)
        e_dev, e_ref = TC.rel_err(got.r.minimizer, ld.x), TC.rel_err(oracle.minimizer, ld.x)
        bound = ac.trajectory_bound(e_ref, k, max(1, f64.iterations))
        assert e_dev <= bound, (label, "x", e_dev, e_ref, bound)
        assert TC.scalar_err(got.r.ssr, ld.ssr) <= ac.trajectory_bound(TC.scalar_err(oracle.ssr, ld.ssr), k, max(1, f64.iterations)), (label, "ssr")
        return
    t = got.trace
    assert [int(v) for v in t["accept"]] == [int(r["accepted"]) for r in f64.its], label
    if inner:
        assert [int(v) for v in t["inner"]] == [int(r["inner"]) for r in f64.its], (label, list(t["inner"]))
    worst, rounding = 0.0, 0
    for i, r64 in enumerate(f64.its):
        if r64["pure_delta"]:       # bit for bit from the delta before it (the start delta where the loop does not rescale it)
            before = t["delta"][i - 1] if i else (start_delta if "delta_scaled_by_wnorm_x" not in r64["labels"] else None)
            if before is not None:
                assert float(t["delta"][i]) == R.pure_delta(r64["pure_op"], before), \
                    (label, i + 1, "delta", r64["pure_op"], float(before), float(t["delta"][i]))
        xd = np.asarray(t["x"][i])
        if np.all(np.isfinite(xd)):
            assert lower is None or np.all(xd >= lower), (label, i + 1, "below the lower bound")
            assert upper is None or np.all(xd <= upper), (label, i + 1, "above the upper bound")
    for i, what, hp, cond, bound in TC.trajectory_pieces(f64, ld, oracle.trace, k):
        dev = t[what][i]
        if what != "x" and np.isnan(LD(hp)):
            assert np.isnan(dev), (label, i + 1, what)
            continue
        e_dev = TC.piece_err(what, dev, hp)
        assert e_dev <= bound, (label, i + 1, what, e_dev, bound, cond)
        if cond > TC.COND_CAP:      # a comparison of rounding errors: made, not counted
            rounding += 1
        else:
            worst = max(worst, e_dev / bound)
    WORST[driver] = max(WORST.get(driver, 0.0), worst)
    print("TRGPU %-44s %-22s iter %2d worst e_dev/bound %.3f, %d comparisons at rounding level (cond > %.0e)"
          % (label, driver, f64.iterations, worst, rounding, TC.COND_CAP))


@pytest.fixture
def arithmetic():
    """Fast kernels for every driver but the *_exact ones; the library's default again afterwards."""
    def choose(driver):
        lsq.set_exact(driver.endswith("_exact"))
    yield choose
    lsq.set_exact(None)


def _three_runs(run):
    prev = lsq.debug_get()
    try:
        lsq.debug_set(None, 0)
        got, again = run(), run()
        lsq.debug_set(None, 1)
        serial = run()
    finally:
        lsq.debug_set(prev[0], prev[1])
    return got, again, serial


def _takes(case, driver):
    if driver == "sharded_world1":
        return case.kind == "lm"
    return True


@pytest.mark.parametrize("driver", HOST_DRIVERS)
@pytest.mark.parametrize("name", NAMES)
def test_case_on_host_callback_driver(ctx, name, driver, arithmetic, monkeypatch):
    case = TC.cases()[name]
    if not _takes(case, driver):
        # the sharded entry is LevenbergMarquardt(LSMR()) only: a Dogleg case is refused with a status (a start outside the
        # bounds is refused first, as everywhere)
        got = run_host_driver(ctx, case, driver, monkeypatch)
        want = lsq._lib.EBOUNDS if "x0_outside" in name else lsq._lib.EARG
        assert got.status == want, (name, got.status)
        return
    kind, osolver = _solver_of(driver)
    z = TC.certify(name, kind)
    orc = oracle_of(name, osolver)
    if TC.summary(orc) != TC.summary(z.f64):
        # a factorisation meets the NaN Jacobian before the loop does: the status is the oracle's with this solver
        assert "nonfinite" in name and osolver == O.CHOLESKY, (name, TC.summary(orc), TC.summary(z.f64))
        arithmetic(driver)
        got = run_host_driver(ctx, case, driver, monkeypatch)
        assert got.status == orc.status != 0, (name, got.status, orc.status)
        return
    arithmetic(driver)
    got, again, serial = _three_runs(lambda: run_host_driver(ctx, case, driver, monkeypatch))
    check_trajectory(name, driver, got, z.f64, z.ld, orc, max(case.m, case.n), kind == "lsmr" and driver != "operator_level",
                     _start_delta(case),
                     lower=case.opts["lower"], upper=case.opts["upper"], traced=driver != "operator_level")
    for other in (again, serial):
        assert other.bits() == got.bits(), (name, driver)


# ------------------------------------------------------------------------------------------------ batched
def run_batched(ctx, case, B, pos, solver):
    """The case as block `pos` of a batch of B; the other blocks are the plain model from starts of their own."""
    p = case.make()
    m, n = case.m, case.n
    x0 = np.zeros(B * n)
    x0.reshape(B, n)[:] = np.array([0.1, -0.05]) + 0.001 * np.arange(B)[:, None]
    x0[pos * n:(pos + 1) * n] = case.x0
    A = TC.A4

    def f_(out, x):
        out.reshape(B, m)[:] = np.tanh(x.reshape(B, n)) @ A.T - TC.B4
        p.f(out[pos * m:(pos + 1) * m], x[pos * n:(pos + 1) * n].copy())

    def g_(J, x):
        t = np.tanh(x.reshape(B, n))
        J.data.reshape(B, n, m)[:] = A.T[None, :, :] * (1 - t * t)[:, :, None]
        D = np.zeros((m, n))
        p.g(D, x[pos * n:(pos + 1) * n].copy())
        J.data[pos * m * n:(pos + 1) * m * n] = D.reshape(-1, order="F")

    o = _opts(case)
    for key, fill in (("lower", -np.inf), ("upper", np.inf)):
        if len(o[key]):
            full = np.full(B * n, fill)
            full[pos * n:(pos + 1) * n] = o[key]
            o[key] = full
    Opt = lsq.LevenbergMarquardt if case.kind == "lm" else lsq.Dogleg
    nls = lsq.LeastSquaresProblem(x=x0, y=np.zeros(B * m), f_=f_, g_=g_, J=lsq.BlockDiagonal(B, m, n))
    try:
        r = lsq.optimize_batched_(nls, Opt(solver()), full_trace=True, ctx=ctx, **o)
    except lsq._lib.LsqError as e:
        return Got(e.status)
    rb = r.block(pos)
    return Got(rb.status, rb)


@pytest.mark.parametrize("solver", ["cholesky", "blockqr"])
@pytest.mark.parametrize("B", [1, 5, 300])
@pytest.mark.parametrize("name", NAMES)
def test_case_as_a_block_of_a_batch(ctx, name, B, solver):
    case = TC.cases()[name]
    z = TC.certify(name)
    osolver = O.CHOLESKY if solver == "cholesky" else O.QR
    orc = oracle_of(name, osolver)
    pos = B // 2
    run = lambda: run_batched(ctx, case, B, pos, lsq.Cholesky if solver == "cholesky" else lsq.BlockQR)   # noqa: E731
    if TC.summary(orc) != TC.summary(z.f64):
        assert "nonfinite" in name and osolver == O.CHOLESKY, (name, TC.summary(orc), TC.summary(z.f64))
        got = run()
        assert got.status == orc.status != 0, (name, got.status, orc.status)
        return
    got, again, serial = _three_runs(run)
    if z.f64.status == R.ENONFINITE:
        # a block that meets a non-finite x is frozen with the status; the reference counts the iteration it completed
        assert got.status == lsq._lib.ENONFINITE and got.r.iterations == z.f64.iterations, (name, got.status)
        return
    check_trajectory("%s B=%d" % (name, B), "batched_" + solver, got, z.f64, z.ld, orc, max(case.m, case.n), False,
                     _start_delta(case),
                     lower=case.opts["lower"], upper=case.opts["upper"])
    for other in (again, serial):
        assert other.bits() == got.bits(), (name, B, solver)


@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("kind", ["lm", "dogleg"])
def test_block_whose_jacobian_turns_nan(ctx, kind, bounded):
    """One block of five whose g! writes a NaN into a Jacobian entry from its third call on, with and without bounds on that
    block, against the oracle on that block alone: the NaN reaches the step, the clip must keep it (Julia's min / max
    propagate NaN), the trial point is non-finite, the step is refused and the block ends with ENONFINITE at the next
    check_isfinite -- with the counts of the reference at that point.  The other blocks finish as if alone."""
    B, pos, m, n = 5, 2, TC.M, TC.N
    lower = np.array([-0.5, -0.5]) if bounded else None
    upper = np.array([0.5, 0.5]) if bounded else None

    class Turning(TC.Model):
        def g(self, J, x):
            super().g(J, x)
            if self.ng >= 3:
                J[1, 0] = np.nan

    case = TC.Case("nan_jacobian", kind, Turning, set(), x0=(0.4, 0.4), iterations=8, lower=lower, upper=upper, **TC.ZERO)
    orc = TC.oracle(case, O.CHOLESKY)
    assert orc.status != 0 and orc.g_calls == 3, (orc.status, orc.g_calls)
    for solver in (lsq.Cholesky, lsq.BlockQR):
        got = run_batched(ctx, case, B, pos, solver)
        if solver is lsq.BlockQR:
            orc_s = TC.oracle(case, O.QR)
        else:
            orc_s = orc
        assert got.status == orc_s.status, (kind, bounded, solver.__name__, got.status, orc_s.status)
        assert (got.r.iterations, got.r.f_calls, got.r.g_calls) == (orc_s.iterations, orc_s.f_calls, orc_s.g_calls), \
            (kind, bounded, solver.__name__)
        assert not got.r.converged


# ------------------------------------------------------------------------------------------------ index spread
def _spread_host_problem(p):
    S = sp.csc_matrix((p.nzval.copy(), p.rowval, p.colptr), shape=(p.m, p.n))
    A = S.copy()

    def f_(out, x):
        out[:] = A @ np.tanh(x) - p.b

    def g_(J, x):
        t = np.tanh(x)
        J.data[:] = p.nzval * np.repeat(1 - t * t, 3)

    return lsq.LeastSquaresProblem(x=p.x0.copy(), y=np.zeros(p.m), f_=f_, g_=g_, J=S)


SPREAD_DRIVERS = ("csc_lsmr", "csc_lsmr_sliced", "csc_lsmr_separate", "model_sliced")


def run_spread(ctx, p, kind, bounded, driver, monkeypatch):
    lo, hi = (p.lower, p.upper) if bounded else ((), ())
    kw = dict(iterations=TC.SPREAD_ITERATIONS, delta=p.delta(kind), **TC.ZERO)
    if driver == "model_sliced":
        monkeypatch.setenv("LSQ_SELL_FORCE", "1")
        try:
            pr = lsq.synthetic.TanhProblem(p.m, p.n, sparse=True, ctx=ctx, inputs=(p.colptr, p.rowval, p.nzval), b=p.b)
        finally:
            monkeypatch.delenv("LSQ_SELL_FORCE")
        try:
            pr.reset(p.x0)
            before = pr.paths()["pair_tails"]
            r = pr.optimize(lsq._lib.LEVENBERG_MARQUARDT if kind == "lm" else lsq._lib.DOGLEG, lsq._lib.LSMR, trace=True,
                            lower=lo if bounded else None, upper=hi if bounded else None, **kw)
            paths = pr.paths()
            # the three-launch LSMR iteration keeps x in LDS: one column window (n = 16384 and beyond have two)
            one_window = lsq.api.mat_layout(pr.J)["srows"]["ncw"] == 1
            assert paths["sliced_rows"] and paths["sliced_cols"], paths
            assert paths["lsmr_path"] == ("three-launch" if one_window else "four-launch"), paths
            # (without bounds the tail is handed to the solve; with bounds tail_ok is false in optimize_lm_loop and the same tail
            #  runs unguarded behind k_box_clip: a condition of the code, no counter tells the two apart)
            if kind == "lm" and one_window:
                assert paths["pair_tails"] > before, paths
            return Got(0, r)
        finally:
            pr.close()
    Opt = lsq.LevenbergMarquardt if kind == "lm" else lsq.Dogleg
    nls = _spread_host_problem(p)
    sliced = driver == "csc_lsmr_sliced"
    if sliced:
        monkeypatch.setenv("LSQ_SELL_FORCE", "1")
    try:
        alloc = lsq.LeastSquaresProblemAllocated(nls, Opt(lsq.LSMR()), ctx=ctx)
    finally:
        if sliced:
            monkeypatch.delenv("LSQ_SELL_FORCE")
    lay = alloc._Jd.layout()
    assert lay["srows"]["active"] == sliced and lay["scols"]["active"] == sliced, lay
    if driver == "csc_lsmr_separate":
        monkeypatch.setenv("LSQ_LSMR_SEPARATE_SETUP", "1")
    try:
        return _guard(lambda: lsq.optimize_(alloc, full_trace=True, lower=lo, upper=hi, **kw))
    finally:
        if driver == "csc_lsmr_separate":
            monkeypatch.delenv("LSQ_LSMR_SEPARATE_SETUP")
        alloc.free()


@pytest.mark.parametrize("driver", SPREAD_DRIVERS)
@pytest.mark.parametrize("bounded", [True, False], ids=["bounded", "free"])
@pytest.mark.parametrize("kind", ["lm", "dogleg"])
@pytest.mark.parametrize("n", TC.SPREAD_N)
def test_index_spread(ctx, n, kind, bounded, driver, arithmetic, monkeypatch):
    """An active bound on the first and last index of every register slot and workgroup of the fast kernels, the largest
    |g_i| of the whole vector on a bounded index: a projection or a clip that misses one index changes maxabs_gr and x."""
    z = TC.certify_spread(n, kind, bounded)
    p = z.problem
    arithmetic(driver)
    got, again, serial = _three_runs(lambda: run_spread(ctx, p, kind, bounded, driver, monkeypatch))
    label = "spread n=%d %s %s" % (n, kind, "bounded" if bounded else "free")
    check_trajectory(label, driver, got, z.f64, z.ld, z.oracle, p.m, True, p.delta(kind),
                     lower=p.lower if bounded else None, upper=p.upper if bounded else None)
    if bounded:
        at = np.where(np.isfinite(p.upper[p.at]), p.upper[p.at], p.lower[p.at])
        assert np.array_equal(np.asarray(got.r.minimizer)[p.at], at), label            # every bounded component ends ON its bound
    for other in (again, serial):
        assert other.bits() == got.bits(), (label, driver)


def test_model_takes_bounds(ctx):
    """TanhProblem.optimize(lower=, upper=): refused when the start is outside, as optimize_ refuses it."""
    p = TC.spread(65)
    pr = lsq.synthetic.TanhProblem(p.m, p.n, sparse=True, ctx=ctx, inputs=(p.colptr, p.rowval, p.nzval), b=p.b)
    try:
        pr.reset(np.ones(p.n))
        with pytest.raises(lsq._lib.ArgumentError) as e:
            pr.optimize(lsq._lib.LEVENBERG_MARQUARDT, lsq._lib.LSMR, lower=p.lower, upper=p.upper)
        assert e.value.status == lsq._lib.EBOUNDS
        with pytest.raises(lsq._lib.ArgumentError):
            pr.optimize(lsq._lib.LEVENBERG_MARQUARDT, lsq._lib.LSMR, lower=p.lower[:-1])
    finally:
        pr.close()


def test_zz_worst_ratio_per_driver():
    """Prints the worst e_dev / bound of every driver that ran in this session (DESIGN section 5 quotes it)."""
    for driver, w in sorted(WORST.items()):
        print("TRWORST %-22s %.3f" % (driver, w))
        assert w <= 1.0
