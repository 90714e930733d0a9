"""The two ends of an LM+LSMR solve of the built-in model on the sliced layouts.

Tail: k_sell_rows_pair takes LM's acceptance test AND the convergence test on the device and opens the gate of the queued
gradient + colsumabs2 pass only behind a step that is accepted and not converged (the host's own decision rules: it adopts the pass
only if it goes on itself).  Head: one n-length launch at x0 (tanh, 1 - tanh^2, the non-finite check), the start residual pass
publishes its two scalars itself and leaves the residual in slice order too, and the first g! with its gradient pass is queued
before the host waits for those scalars.

None of this may change a bit of a result.  The comparator is the same library with the speculative pass switched off
(LSQ_NO_SPEC_GRADIENT=1: identical bits asked) and with the two-pass tail (LSQ_NO_PAIR_TAIL=1: the sums of squares are associated
differently there, 1e-12 as in test_lm_pair_tail_matches_the_two_passes).

Shape: 160000 x 2000 with 600 entries per column, nnz 1.2e6 -- just above both activation thresholds of the sliced layouts
(nnz >= 2^20, m > 131072; rows average 7.5 entries: the stream plan), n <= 10200 for the pair tail, 40 row blocks."""
import numpy as np
import pytest

lsq = pytest.importorskip("lsq_amd")

pytestmark = pytest.mark.gpu

M, N, PER_COL, SEED = 160000, 2000, 600, 29
L = lsq._lib


@pytest.fixture(scope="module")
def inputs():
    """Pattern, values and right-hand side (the generator's default: x_true ~ U(-1, 1), noise 1e-3), drawn once."""
    cp, rv, nz = lsq.synthetic.sparse_inputs(M, N, PER_COL, SEED)
    _, b = lsq.synthetic.rhs_for(lambda t: lsq.synthetic.csc_matvec(M, cp, rv, nz, t), M, N, SEED)
    return (cp, rv, nz), b


def _problem(ctx, inputs):
    return lsq.synthetic.TanhProblem(M, N, sparse=True, per_col=PER_COL, seed=SEED, ctx=ctx, inputs=inputs[0], b=inputs[1])


def _summary(pr, r):
    """Everything a caller can see of a solve: counts, flags, scalars, the traced iterates and the residual vector."""
    out = [r.iterations, r.converged, r.x_converged, r.f_converged, r.g_converged, r.f_calls, r.g_calls, r.mul_calls,
           r.lsmr_iterations, r.ssr, r.minimizer, pr.fcur.get()]
    if r.trace is not None:
        out += [np.array(r.trace[k]) for k in ("inner", "accept", "ssr", "gnorm", "delta", "x")]
    return out


def _same(a, b, what):
    assert len(a) == len(b)
    for k, (u, v) in enumerate(zip(a, b)):
        if isinstance(u, np.ndarray):
            assert np.array_equal(u, v), (what, k, float(np.abs(u - v).max()))
        else:
            assert u == v, (what, k, u, v)


def _solve(ctx, inputs, monkeypatch, env=None, x0=None, **kw):
    """One solve on a fresh problem object under the given environment switches (read per run by the library)."""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    try:
        pr = _problem(ctx, inputs)
        try:
            pr.reset(x0)
            r = pr.optimize(L.LEVENBERG_MARQUARDT, L.LSMR, **kw)
            return _summary(pr, r)
        finally:
            pr.close()
    finally:
        for k in (env or {}):
            monkeypatch.delenv(k)


NO_SPEC = {"LSQ_NO_SPEC_GRADIENT": "1"}
NO_PAIR = {"LSQ_NO_PAIR_TAIL": "1"}


def _case_default_tolerances(ctx, inputs, monkeypatch):
    a = _solve(ctx, inputs, monkeypatch, trace=True)
    b = _solve(ctx, inputs, monkeypatch, env=NO_SPEC, trace=True)
    assert a[1] and 2 <= a[0] < 1000, a[:5]                     # a converging solve of several steps
    assert a[13][a[0] - 1] == 1                                 # ... whose last step is an accepted one (the gated case)
    _same(a, b, "default vs no speculative pass")
    c = _solve(ctx, inputs, monkeypatch, env=NO_PAIR, trace=True)
    _same(a[:9], c[:9], "default vs two-pass tail: counts and flags")
    _same(a[12:14], c[12:14], "default vs two-pass tail: inner counts, accept pattern")
    assert np.allclose(a[14], c[14], rtol=1e-12, atol=0) and a[9] == pytest.approx(c[9], rel=1e-12)
    assert np.max(np.abs(a[17] - c[17])) <= 1e-12 and np.max(np.abs(a[10] - c[10])) <= 1e-12
    assert np.max(np.abs(a[11] - c[11])) <= 1e-12 * max(1.0, np.max(np.abs(c[11])))
    return a


def _case_two_solves(ctx, inputs, fresh):
    pr = _problem(ctx, inputs)
    try:
        runs = []
        for _ in range(2):
            pr.reset()
            runs.append(_summary(pr, pr.optimize(L.LEVENBERG_MARQUARDT, L.LSMR, trace=True)))
    finally:
        pr.close()
    _same(runs[0], fresh, "first solve of a reused object vs a fresh object")
    _same(runs[1], runs[0], "second solve vs first solve on one object")


def test_default_tolerances_match_the_unspeculated_and_the_two_pass_runs(ctx, inputs, monkeypatch):
    """Case 1: default tolerances from x0 = 0, traced.  The converging last step is accepted: the device closes the gate there."""
    _case_default_tolerances(ctx, inputs, monkeypatch)


def test_two_solves_in_a_row_on_one_object(ctx, inputs, monkeypatch):
    """Case 2: a stale adopted pass, stale tanh / factor records or a stale slice-order mirror would show in the second solve."""
    fresh = _solve(ctx, inputs, monkeypatch, trace=True)
    _case_two_solves(ctx, inputs, fresh)


def test_one_iteration_and_a_start_at_the_minimizer(ctx, inputs, monkeypatch):
    """Case 3: iterations=1 (no pass may be queued behind the only step), and a solve started at a converged minimizer (its first
    step converges: the gate stays shut behind the very first tail)."""
    a = _solve(ctx, inputs, monkeypatch, iterations=1, trace=True)
    b = _solve(ctx, inputs, monkeypatch, env=NO_SPEC, iterations=1, trace=True)
    assert a[0] == 1 and not a[1]
    _same(a, b, "iterations=1")
    xmin = _solve(ctx, inputs, monkeypatch)[10]
    a = _solve(ctx, inputs, monkeypatch, x0=xmin, trace=True)
    b = _solve(ctx, inputs, monkeypatch, env=NO_SPEC, x0=xmin, trace=True)
    assert a[0] == 1 and a[1], a[:5]
    _same(a, b, "start at the minimizer")


def test_rejected_steps_with_zero_tolerances(ctx, inputs, monkeypatch):
    """Case 4: zero tolerances, 8 iterations, a huge first radius from a start in tanh's flat region (x0 ~ U(-3, 3): the
    Gauss-Newton-like steps overshoot; the CPU oracle accepts steps 1, 4, 5, 6, 8 and refuses 2, 3, 7): refused steps, gates that
    stay shut, passes that run and are adopted -- identical to the run without the speculative pass."""
    kw = dict(iterations=8, delta=1e6, x_tol=0, f_tol=0, g_tol=0, trace=True, x0=lsq.synthetic.uniform(N, 7, -3.0, 3.0))
    a = _solve(ctx, inputs, monkeypatch, **kw)
    b = _solve(ctx, inputs, monkeypatch, env=NO_SPEC, **kw)
    assert a[0] == 8 and not np.all(a[13] == 1) and np.any(a[13] == 1), a[13]
    _same(a, b, "rejections")


def test_nonfinite_start_leaves_the_problem_usable(ctx, inputs, monkeypatch):
    """Case 5: x0 with a NaN at index 7 -> IsFiniteException with that index; the same object then solves from x0 = 0 exactly
    as a fresh one does (nothing of the work queued ahead for the refused x0 may survive)."""
    fresh = _solve(ctx, inputs, monkeypatch, trace=True)
    pr = _problem(ctx, inputs)
    try:
        x0 = np.zeros(N)
        x0[7] = np.nan
        pr.reset(x0)
        with pytest.raises(lsq.IsFiniteException) as ei:
            pr.optimize(L.LEVENBERG_MARQUARDT, L.LSMR, trace=True)
        assert str(ei.value).endswith("non-finite x at index 7"), str(ei.value)     # (the native loop's message names the index)
        pr.reset()
        again = _summary(pr, pr.optimize(L.LEVENBERG_MARQUARDT, L.LSMR, trace=True))
    finally:
        pr.close()
    _same(again, fresh, "solve after a refused x0 vs a fresh object")


@pytest.mark.parametrize("mode", ["serial", "jitter"])
def test_debug_modes(ctx, inputs, monkeypatch, mode):
    """Case 6: cases 1 and 2 with every launch waited for, and with random host stalls of up to 100 us in front of the launches
    (whatever holds only because the next launch follows at once fails under them).  Both must also give the bits of the
    normal mode."""
    prev = lsq.debug_get()
    try:
        lsq.debug_set(0, 0)
        normal = _solve(ctx, inputs, monkeypatch, trace=True)
        if mode == "serial":
            lsq.debug_set(0, 1)
        else:
            lsq.debug_set(100, 0)
        a = _case_default_tolerances(ctx, inputs, monkeypatch)
        _same(a, normal, "debug mode vs normal mode")
        _case_two_solves(ctx, inputs, a)
    finally:
        lsq.debug_set(prev[0], prev[1])
