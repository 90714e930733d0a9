"""Robust loss tier without a device: the numpy twin of the transform (lsq_amd.loss_transform) against its longdouble
reference, planted mistakes that the same checks must reject, and the CPU oracle's optimize on the wrapped host problem
(lsq_amd.robust_twin) of the cases of tests/robust_loss_common.py: it converges, and at its x an independent evaluation of
J'(rho' f / sigma^2) from the RAW f_ and g_ is within g_tol plus the rounding bound of that product.  The runs use
x_tol = f_tol = 0, so that the gradient is what ends them, and g_tol = robust_loss_common.gradient_tolerance."""
import numpy as np
import pytest

import accuracy_common as ac
import robust_loss_common as R
import lsq_amd as lsq
from oracle import oracle as O

SCALES = (1.0, 0.37, 8.0)


def all_inputs(c, extremes=False):
    return np.concatenate([R.transform_inputs(c), R.grid_inputs(c)] + ([R.extreme_inputs(c)] if extremes else []))


# ------------------------------------------------------------------------------------------------ the transform
@pytest.mark.parametrize("loss", R.LOSSES)
@pytest.mark.parametrize("c", SCALES)
@pytest.mark.parametrize("weighted", [False, True])
def test_transform_against_longdouble(loss, c, weighted):
    f = all_inputs(c, extremes=not weighted)
    sigma = 10.0 ** np.random.default_rng(7).uniform(-1.5, 1.5, f.size) if weighted else None
    rt, rowf = lsq.loss_transform(f, loss, c, sigma)
    e_rt, e_w, e_sq = R.transform_errors(rt, rowf, f, loss, c, sigma)
    print("ROBUST twin %s c=%g sigma=%s | e_rt %.3e e_w %.3e e_sq %.3e bound %.3e" % (loss, c, weighted, e_rt, e_w, e_sq, ac.bound(0.0, 1)))
    assert e_rt <= ac.bound(0.0, 1) and e_w <= ac.bound(0.0, 1)
    assert e_sq <= 2.0 * ac.bound(0.0, 1)                     # (a square: twice the relative error)
    assert R.nonfinite_classes_kept(rt, f)
    fin = np.isfinite(f)
    z = f if sigma is None else f / sigma
    w = rowf if sigma is None else rowf * sigma
    assert np.all((w >= 0.0) & (w <= 1.0 + (4e-16 if weighted else 0.0)))     # (times sigma again: one more rounding)
    assert np.all(np.abs(rt[fin]) <= np.abs(z[fin]))
    assert np.array_equal(np.signbit(rt[fin]), np.signbit(z[fin]))            # signed zeros included


@pytest.mark.parametrize("loss", R.LOSSES)
@pytest.mark.parametrize("c", SCALES)
def test_transform_is_monotone(loss, c):
    f = all_inputs(c, extremes=True)
    f = np.sort(np.abs(f[np.isfinite(f)]))
    rt, rowf = lsq.loss_transform(f, loss, c)
    assert np.all(np.diff(rt) >= 0.0)
    m = -f
    assert np.array_equal(lsq.loss_transform(m, loss, c)[0], -rt)


@pytest.mark.parametrize("loss", ["huber", "soft_l1", "cauchy"])
def test_planted_mistakes_are_caught(loss):
    """The IRLS factor sqrt(rho') in place of w, and a missing 1 / sigma: both must fail the derivative check."""
    c = 0.37
    f = all_inputs(c)
    sigma = 10.0 ** np.random.default_rng(7).uniform(-1.5, 1.5, f.size)
    rt, rowf = lsq.loss_transform(f, loss, c, sigma)
    with np.errstate(all="ignore"):
        irls = np.sqrt(R.rho_prime((f / (sigma * c)) ** 2, loss)) / sigma
    assert R.transform_errors(rt, irls, f, loss, c, sigma)[1] > 1e3 * ac.bound(0.0, 1)
    assert R.transform_errors(rt, rowf * sigma, f, loss, c, sigma)[1] > 1e3 * ac.bound(0.0, 1)
    # ... and a residual that was not divided by sigma fails the value check
    assert R.transform_errors(lsq.loss_transform(f, loss, c)[0], rowf, f, loss, c, sigma)[0] > 1e3 * ac.bound(0.0, 1)


def test_transform_refusals():
    f = np.ones(3)
    with pytest.raises(lsq.ArgumentError):
        lsq.loss_transform(f, "tukey")
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(lsq.ArgumentError):
            lsq.loss_transform(f, "huber", bad)
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(lsq.ArgumentError, match="entry 1"):
            lsq.loss_transform(f, "huber", 1.0, np.array([1.0, bad, 1.0]))
    with pytest.raises(lsq.DimensionMismatch):
        lsq.loss_transform(f, "huber", 1.0, np.ones(4))


def test_header_and_bindings_know_the_new_entries():
    import julia_shim_lint as JL
    names = ("lsq_mat_scale_rows", "lsq_loss_create", "lsq_loss_destroy", "lsq_loss_set_problem", "lsq_loss_f", "lsq_loss_g",
             "lsq_loss_eval")
    declared, L = lsq.declared_symbols(), lsq.lib()
    protos = JL.header_prototypes()
    bound = {c[0] for c in JL.ccalls()}
    for n in names:
        assert n in declared and hasattr(L, n) and n in L._signatures and n in protos and n in bound, n
    assert protos["lsq_loss_create"][1][-1] == "ptrptr" and protos["lsq_loss_eval"][1][0] == "ptr:void"
    hdr = open(JL.HEADER).read()
    assert "lsq_mat_scale_rows" in hdr[hdr.index("FRESHNESS CONTRACT"):hdr.index("int lsq_mat_refresh")]


# ------------------------------------------------------------------------------------------------ the oracle on the wrapped problem
ORACLE_GRID = {
    "decay": [(o, s) for o in ("dogleg", "lm") for s in ("qr", "cholesky", "lsmr")],
    # the oracle's direct solvers take dense matrices only: they get `line` as a dense copy.  Its empty column makes
    # Dogleg(Cholesky()) a RankDeficientException with or without a loss (asserted below); everything else runs
    "line": [("dogleg", "lsmr"), ("lm", "lsmr")],
    "line dense": [("dogleg", "qr"), ("lm", "qr"), ("lm", "cholesky"), ("dogleg", "lsmr"), ("lm", "lsmr")],
}


def make_case(name):
    return R.line_case(dense=True) if name == "line dense" else R.CASES[name]()


OPT = {"dogleg": O.DOGLEG, "lm": O.LM}
SOL = {"qr": O.QR, "cholesky": O.CHOLESKY, "lsmr": O.LSMR}


def oracle_run(case, loss, c, sigma, opt, sol, **kw):
    rf, rg = lsq.robust_twin(case.f_, case.g_, loss, c, sigma)
    mat, f, g = R.oracle_problem(O, case, rf, rg)
    return O.optimize(OPT[opt], SOL[sol], mat, case.x0, f, g, **kw)


@pytest.mark.parametrize("name,opt,sol", [(n, o, s) for n, grid in ORACLE_GRID.items() for o, s in grid])
@pytest.mark.parametrize("loss", ["huber", "soft_l1", "cauchy", "linear"])
def test_oracle_converges_to_a_stationary_point_of_the_robust_cost(name, opt, sol, loss):
    case = make_case(name)
    c = 2.0
    g_tol = R.gradient_tolerance(case, loss, c, case.sigma)
    r = oracle_run(case, loss, c, case.sigma, opt, sol, x_tol=0.0, f_tol=0.0, g_tol=g_tol)
    assert r.status == 0 and r.converged and r.g_converged, (r.status, r.iterations)
    grad, gmax, bound = R.robust_gradient(case, R.measured_point(r, case.x0), loss, c, case.sigma)
    print("ROBUST oracle %s %s/%s %s | %d iterations, g_tol %.3e, |grad|_inf %.3e, product bound %.3e"
          % (name, opt, sol, loss, r.iterations, g_tol, gmax, float(np.max(bound))))
    assert np.all(np.abs(grad) <= g_tol + bound)
    assert abs(gmax - r.trace["gnorm"][-1]) <= float(np.max(bound))     # the loop's J~'r~ IS that gradient
    assert R.robust_gradient(case, r.minimizer, loss, c, case.sigma)[1] <= R.LAST_STEP_FACTOR * g_tol   # ... and at the returned x
    # the cost the loop reports is c^2 sum(rho) of the raw residual there
    f = np.zeros(case.m)
    case.f_(f, r.minimizer)
    rho = R.reference(f, loss, c, case.sigma)[2]
    assert abs(r.ssr - float(c * c * np.sum(rho))) <= 1e-12 * r.ssr


def test_the_one_pair_the_empty_column_excludes():
    case = R.line_case(dense=True)
    mat, f, g = R.oracle_problem(O, case, case.f_, case.g_)
    assert O.optimize(O.DOGLEG, O.CHOLESKY, mat, case.x0, f, g).status == 3            # LSQ_ERANK, no loss involved
    assert oracle_run(case, "huber", 2.0, case.sigma, "dogleg", "cholesky").status == 3


@pytest.mark.parametrize("name,opt,sol", [("decay", "dogleg", "qr"), ("decay", "lm", "cholesky"), ("line", "lm", "lsmr")])
def test_huber_with_a_huge_scale_is_the_plain_run(name, opt, sol):
    case = R.CASES[name]()
    mat, f, g = R.oracle_problem(O, case, case.f_, case.g_)
    plain = O.optimize(OPT[opt], SOL[sol], mat, case.x0, f, g)
    rob = oracle_run(case, "huber", 1e300, None, opt, sol)
    assert_same_run(plain, rob)


@pytest.mark.parametrize("name,opt,sol", [("decay", "dogleg", "qr"), ("decay", "lm", "cholesky"), ("line", "lm", "lsmr")])
def test_linear_with_sigmas_is_the_hand_weighted_problem(name, opt, sol):
    """Hand-weighted: f / sigma, and J times the ONE rounded factor 1 / sigma per row (what the handle stores)."""
    case = R.CASES[name]()
    inv = 1.0 / case.sigma

    def hf(o, x):
        case.f_(o, x)
        o[:] = o / case.sigma

    def hg(J, x):
        case.g_(J, x)
        lsq.api._scale_rows_host(J, inv)

    mat, f, g = R.oracle_problem(O, case, hf, hg)
    hand = O.optimize(OPT[opt], SOL[sol], mat, case.x0, f, g)
    rob = oracle_run(case, "linear", 1.0, case.sigma, opt, sol)
    assert_same_run(hand, rob)


def assert_same_run(a, b):
    assert a.status == b.status == 0
    for k in ("iterations", "converged", "x_converged", "f_converged", "g_converged", "f_calls", "g_calls", "mul_calls", "ssr"):
        assert getattr(a, k) == getattr(b, k), k
    assert np.array_equal(a.minimizer, b.minimizer) and np.array_equal(a.fcur, b.fcur)
    for k in a.trace:
        assert np.array_equal(a.trace[k], b.trace[k]), k


# ------------------------------------------------------------------------------------------------ robust_twin on every container
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_robust_twin_scales_every_container_by_rows(name):
    case = R.CASES[name]()
    x = case.x0 + 0.01
    rf, rg = lsq.robust_twin(case.f_, case.g_, "soft_l1", 0.5, case.sigma)
    raw, J0, J1 = np.zeros(case.m), case.new_J(), case.new_J()
    case.f_(raw, x)
    case.g_(J0, x)
    rg(J1, x)
    rt, rowf = lsq.loss_transform(raw, "soft_l1", 0.5, case.sigma)
    out = np.zeros(case.m)
    rf(out, x)
    assert np.array_equal(out, rt)
    D0 = J0 if case.kind == "dense" else J0.toarray()
    D1 = J1 if case.kind == "dense" else J1.toarray()
    assert np.array_equal(D1, D0 * rowf[:, None])
    assert lsq.robust_twin(case.f_, None, "huber")[1] is None
