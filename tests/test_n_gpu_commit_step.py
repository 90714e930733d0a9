"""The launch that commits the expected stop of an LM inner solve and takes the step: k_lsmr_commit_step (lsq_lsmr3.h).

Where the three-launch LSMR driver expects the stop (the predicted last iteration; iteration 1 when nothing is known yet) and
its caller is the LM loop, one narrow launch decides the iteration instead of a cautious k_lsmr_fused launch.  If the solve is
over it commits what the update workgroups would have committed and takes x_trial = x - dx (tanh, 1 - tanh^2, max|dx|, the
non-finite index) itself; if not, it writes nothing and an ordinary launch commits the iteration again.  None of this may change a
bit: the comparator is the same library with LSQ_NO_COMMIT_STEP=1 (cautious launches and k_step, as before), every trace array,
the counts, x and the residual vector with numpy.array_equal.  Which hand-off a run took is read from
Context.commit_step_stats(), never assumed.

Shapes: the tanh model at 4000 x 129 (300 entries per column, seed 31) with the sliced layouts forced, as in
tests/test_m_gpu_stream_heads.py (its environment; its comparison with the CPU oracle, same tolerances: counts and inner counts
equal, ssr to 1e-12 relative, every traced iterate to 1e-8 * max(1, |x|)).  The oracle's inner counts on that problem are
1, 1, 1, 7, 5, 2: the first solve has nothing to go by and stops at iteration 1 (a commit launch that finds it over), the fourth is
guessed at 1 from the third and goes on to 7 (a commit launch that finds it unfinished -- whatever the timing: the hints that
could replace the guess are published from launch 2 on only).  A stop that an ordinary launch commits is taken from the
589 x 2049 run, where ten of twelve stops come at an iteration nobody guessed.
n = 1, 1023, 1024, 1025, 2049 at m = 589 (6 entries per column): one thread of one workgroup, a partly filled workgroup, exactly
one, one element into the second, two and one element -- the edges of the one-group-per-workgroup mapping and of the ticket round
over 1, 2 and 3 workgroups.
The non-finite step: the same pattern with values scaled by 1e-159, b = 1e152 and Delta = 1e-3 -- one inner iteration whose
P .* x overflows in some elements (the CPU oracle: IsFiniteException at index 36, not at 0), taken by the commit launch."""
import contextlib
import functools
import os

import numpy as np
import pytest

from gpu_common import OPT, SOL, lsq
from oracle import oracle as O
from test_m_gpu_stream_heads import ENV

pytestmark = pytest.mark.gpu

L = lsq._lib
SM, SN, SPER, SSEED = 4000, 129, 300, 31
EM, EPER = 589, 6
KEYS = ("x", "ssr", "delta", "inner", "accept", "gnorm", "rho")
SWITCH = {"LSQ_NO_COMMIT_STEP": "1"}


@pytest.fixture()
def sliced(monkeypatch):
    for k, v in ENV.items():
        monkeypatch.setenv(k, v)
    lsq.set_exact(False)
    yield
    lsq.set_exact(None)


@contextlib.contextmanager
def environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _summary(pr, r):
    return [r.iterations, r.converged, r.f_calls, r.g_calls, r.mul_calls, r.lsmr_iterations, r.ssr, r.minimizer,
            pr.fcur.get()] + [np.array(r.trace[k]) for k in KEYS]


def _solve(ctx, shape=(SM, SN, SPER, SSEED), env=None, x0=None, solves=1, optimizer=L.LEVENBERG_MARQUARDT, path="three-launch",
           inputs=None, b=None, **kw):
    """`solves` traced solves on one problem object: [(summary, commit launches that found the solve over, ... unfinished)]."""
    m, n, per, seed = shape
    out = []
    with environment(env or {}):
        pr = lsq.synthetic.TanhProblem(m, n, sparse=True, per_col=per, seed=seed, ctx=ctx, inputs=inputs, b=b)
        try:
            for _ in range(solves):
                pr.reset(x0)
                before = ctx.commit_step_stats()
                r = pr.optimize(optimizer, L.LSMR, trace=True, **kw)
                after = ctx.commit_step_stats()
                paths = pr.paths()
                assert paths["sliced_rows"] and paths["sliced_cols"] and (path is None or paths["lsmr_path"] == path), paths
                out.append((_summary(pr, r), after[0] - before[0], after[1] - before[1], r))
        finally:
            pr.close()
    return out


def _same(a, b, what):
    assert len(a) == len(b)
    for k, (u, v) in enumerate(zip(a, b)):
        if isinstance(u, np.ndarray):
            assert u.shape == v.shape and np.array_equal(u, v), (what, k)
        else:
            assert u == v, (what, k, u, v)


def _both(ctx, what, **kw):
    """The same solves with commit launches and with the switch set: bit-equal; the switched run launches none."""
    env = kw.pop("env", None) or {}
    a, b = _solve(ctx, env=env, **kw), _solve(ctx, env=dict(env, **SWITCH), **kw)
    for (sa, over, unfinished, _), (sb, o2, u2, _) in zip(a, b):
        print("%s: commit launches that found the solve over %d, unfinished %d; of %d solves" % (what, over, unfinished, sa[0]))
        assert (o2, u2) == (0, 0), what
        _same(sa, sb, what)
    return a


@functools.lru_cache(maxsize=None)
def _oracle():
    cp, rv, nz = lsq.synthetic.sparse_inputs(SM, SN, SPER, SSEED)
    _, b = lsq.synthetic.rhs_for(lambda t: lsq.synthetic.csc_matvec(SM, cp, rv, nz, t), SM, SN, SSEED)
    A = O.Mat(csc=(SM, SN, cp, rv, nz))
    Jo = O.Mat(csc=(SM, SN, cp, rv, np.zeros_like(nz)))
    f, g, ud, keep = O.tanh_model(A, b)
    return O.optimize(OPT["lm"][1], SOL["lsmr"][1], Jo, np.zeros(SN), f, g, ud=ud)


def _against_oracle(r):
    ro = _oracle()
    assert (r.iterations, r.mul_calls, r.f_calls, r.g_calls, r.converged) == \
           (ro.iterations, ro.mul_calls, ro.f_calls, ro.g_calls, ro.converged)
    assert np.array_equal(r.trace["inner"], ro.trace["inner"])
    assert r.ssr == pytest.approx(ro.ssr, rel=1e-12)
    for k in range(ro.iterations):
        xr = ro.trace["x"][k]
        assert np.max(np.abs(r.trace["x"][k] - xr)) <= 1e-8 * max(1.0, np.max(np.abs(xr))), k


def test_default_against_the_switch_and_the_oracle(ctx, sliced):
    (s, over, unfinished, r), = _both(ctx, "default")
    assert s[1] and s[0] >= 2, s[:6]
    assert over >= 1 and unfinished >= 1 and over <= s[0], (over, unfinished)     # (both outcomes of a commit launch: see above)
    _against_oracle(r)


def test_two_solves_on_one_object(ctx, sliced):
    """The second solve's record tags, ticket counter, double-buffered sets and tanh records come from the first."""
    first, second = _both(ctx, "two solves", solves=2)
    _same(first[0], second[0], "second solve vs first solve on one object")
    assert first[1] >= 1 and second[1] >= 1
    _against_oracle(second[3])


def test_a_stop_that_an_ordinary_launch_commits(ctx, sliced):
    """A run with both kinds of stop: taken by a commit launch (no k_step) and committed by an ordinary k_lsmr_fused launch
    (k_step behind it), besides commit launches that found their solve unfinished."""
    (s, over, unfinished, _), = _both(ctx, "589 x 2049", shape=(EM, 2049, EPER, 1000 + 2049), iterations=12)
    assert s[0] == 12
    assert over >= 1 and unfinished >= 1 and s[0] - over >= 1, (s[0], over, unfinished)


def test_one_iteration_and_a_start_at_the_minimizer(ctx, sliced):
    (s, over, unfinished, _), = _both(ctx, "iterations=1", iterations=1)
    assert s[0] == 1 and not s[1]
    assert (over, unfinished) == (1, 0)         # (nothing known, the solve stops at iteration 1: the commit launch takes the only step)
    xmin = _solve(ctx)[0][0][7]
    (s, over, unfinished, _), = _both(ctx, "start at the minimizer", x0=xmin)
    assert s[0] == 1 and s[1], s[:6]
    assert over + unfinished >= 1


def test_rejected_steps(ctx, sliced):
    """Zero tolerances, 8 iterations, a huge first radius from a start in tanh's flat region (tests/test_l_gpu_solve_ends.py,
    case 4): refused steps, after which x is restored from the x_trial and dx the commit launch left."""
    (s, over, unfinished, _), = _both(ctx, "rejections", x0=lsq.synthetic.uniform(SN, 7, -3.0, 3.0), iterations=8, delta=1e6,
                                      x_tol=0, f_tol=0, g_tol=0)
    accept = s[9 + KEYS.index("accept")]
    assert s[0] == 8 and not np.all(accept == 1) and np.any(accept == 1), accept
    assert over >= 1


def test_a_step_that_leaves_x_trial_non_finite(ctx, sliced):
    cp, rv, nz = lsq.synthetic.sparse_inputs(SM, SN, SPER, SSEED)
    kw = dict(inputs=(cp, rv, nz * 1e-159), b=np.full(SM, 1e152), delta=1e-3, iterations=3)
    msgs = []
    for env in ({}, SWITCH):
        before = ctx.commit_step_stats()
        with pytest.raises(lsq.IsFiniteException) as ei:
            _solve(ctx, env=env, **kw)
        after = ctx.commit_step_stats()
        msgs.append((str(ei.value), after[0] - before[0], after[1] - before[1]))
    print(msgs)
    assert msgs[0][0] == msgs[1][0] and msgs[0][0].endswith("non-finite x at index 36"), msgs
    assert msgs[0][1:] == (1, 0) and msgs[1][1:] == (0, 0), msgs       # (the commit launch took that step)


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2049])
def test_edges_of_the_workgroup_mapping(ctx, sliced, n):
    (s, over, unfinished, _), = _both(ctx, "589 x %d" % n, shape=(EM, n, EPER, 1000 + n), iterations=12)
    assert over >= 1, (over, unfinished)


@pytest.mark.parametrize("mode", ["serial", "jitter"])
def test_debug_modes(ctx, sliced, mode):
    """Every launch waited for (no guesses, hence no commit launches), and host stalls of up to 100 us in front of the launches:
    the bits of the normal mode."""
    prev = lsq.debug_get()
    try:
        lsq.debug_set(0, 0)
        normal = _solve(ctx)[0][0]
        lsq.debug_set(*((0, 1) if mode == "serial" else (100, 0)))
        (s, over, unfinished, _), = _both(ctx, mode)
        _same(s, normal, "debug mode vs normal mode")
        assert (over + unfinished == 0) if mode == "serial" else over >= 1
    finally:
        lsq.debug_set(prev[0], prev[1])


def test_other_drivers_launch_none(ctx, sliced):
    """The four-launch iteration and Dogleg's undamped solves hand over no step: counters at zero, results as with the switch."""
    (s, over, unfinished, r), = _both(ctx, "four launches", env={"LSQ_LSMR_FOUR_LAUNCHES": "1"}, path="four-launch")
    assert (over, unfinished) == (0, 0)
    _against_oracle(r)
    (s, over, unfinished, _), = _both(ctx, "Dogleg + LSMR", optimizer=L.DOGLEG, path=None)
    assert (over, unfinished) == (0, 0) and s[0] >= 2
