"""The trust-region cases: every branch of levenberg_marquardt.jl:39-144 and dogleg.jl:41-203 that the tier certifies, each
case naming the branches (labels of tests/trust_region_reference.py) it is there for.

Toy cases are all 4 x 2, so that any of them can sit as one block of a batch.  Two kinds of problem:
  (a) model     r(x) = A tanh(x) - b with its Jacobian (`lie`: g! returns the NEGATED Jacobian, which gives rejections only;
                `bad`: the f! calls, counted from 0, that return 4 r(x) -- a trial the loop must refuse)
  (b) scripted  f! / g! return prescribed vectors per call.  With J = [I; 0] and integer residuals ssr, trial_ssr,
                predicted_ssr and so rho are exact in any summation order.  Host-callback drivers only.

Not reached, with the reason (tests/test_trust_region_host.py prints them in its coverage table):
  clamp_high in LM          colsumabs2[i] <= sum = n * mean < 1e32 * mean for every finite Jacobian with n < 1e32
  beta_cc_nonpositive       with an exact Gauss-Newton step cc = a.(b - a) >= 0 (Cauchy-Schwarz), = 0 only where a = b, where
                            case 3 is not entered; the host tier runs a bounded search over rounding
A non-finite point after an ACCEPTED step comes from overflow, not from a non-finite step: J = 2^-510 [I; 0], f = (2^511, 0,
0, 0), x0 = (-1.9 * 2^1023, 0): the step is about 2^1021 (LM, delta = 1e6) or 2^1021 exactly (Dogleg, case 1), finite, the
scripted trial (2^509, 0, 0, 0) gives rho = 0.9375, the step is accepted and x - dx is -inf: check_isfinite ends the run at the
top of iteration 2.  (The longdouble twin keeps x in float64's range, where the reference's x lives.)
Not here: rho exactly equal to MIN_STEP_QUALITY (strict in LM, non-strict in Dogleg).  1e-3 is not dyadic, so no residuals
make rho that number in every precision: a quotient such as 1 / 1000 rounds to the double 1e-3 in float64 only, and the
longdouble twin, whose quotient is another number, cannot certify the case.

Index-spread cases (spread(n)): r(x) = A tanh(x) - b on a three-band A (rows j, j + 1, j + 3 of column j; m = n + 3), every
column's data different, x0 = 0, bounds infinite except at 0, 255, 256, 1023, 1024, 2047, 2048, 15359, 15360 and n - 1 (the first and last
index of register slots 0, 1 and 15 of the one-workgroup kernels, the edge between slots 1 and 2, and of a 256-thread block of
k_gradnorm / k_box_clip), each half-way between x0 and
the minimizer of the noise-free data, and the columns at those indices four times as large as the others, so that the largest |g_i| sits on an
actively bounded index.  Zero tolerances and a fixed iteration count: the loop runs to `iterations`.
"""
import functools

import numpy as np

import trust_region_reference as R

LD = np.longdouble
M, N = 4, 2
J0 = np.array([[1.0, 0.0], [0.0, 1.0], [0.0, 0.0], [0.0, 0.0]])
A4 = np.array([[1.0, 0.5], [0.25, 1.0], [0.5, -0.75], [-0.3, 0.2]])
XT4 = np.array([0.3, -0.2])
B4 = A4 @ np.tanh(XT4) + 0.01 * np.array([1.0, -1.0, 1.0, 1.0])
A_SKEW = np.array([[1.0, 1.0], [1.0, 1.125], [1.0, 0.875], [0.0, 0.125]])       # nearly parallel columns: case 3 exists
B_SKEW = A_SKEW @ np.tanh(XT4) + 0.01 * np.array([1.0, -1.0, 1.0, 1.0])
SPREAD_N = (1, 63, 64, 65, 1023, 1024, 1025, 16384, 16385)
SPREAD_AT = (0, 255, 256, 1023, 1024, 2047, 2048, 15359, 15360)
SPREAD_ITERATIONS = 4


class Scripted:
    """f! call k returns fs[min(k, last)], g! call k writes Js[min(k, last)]."""

    def __init__(self, fs, Js=(J0,)):
        self.fs = [np.asarray(v, dtype=np.float64) for v in fs]
        self.Js = [np.asarray(v, dtype=np.float64) for v in Js]
        self.nf = self.ng = 0

    def f(self, out, x):
        out[:] = self.fs[min(self.nf, len(self.fs) - 1)]
        self.nf += 1

    def g(self, J, x):
        J[:] = self.Js[min(self.ng, len(self.Js) - 1)]
        self.ng += 1


class Model:
    """r(x) = A tanh(x) - b on a dense A."""

    def __init__(self, A=A4, b=B4, lie=False, bad=()):
        self.A, self.b, self.lie, self.bad = A, b, lie, set(bad)
        self.nf = self.ng = 0

    def f(self, out, x):
        T = out.dtype.type
        out[:] = self.A.astype(out.dtype) @ np.tanh(x) - self.b.astype(out.dtype)
        if self.nf in self.bad:
            out *= T(4)
        self.nf += 1

    def g(self, J, x):
        t = np.tanh(x)
        J[:] = self.A.astype(J.dtype) * (1 - t * t)
        if self.lie:
            J *= -1
        self.ng += 1


class Case:
    def __init__(self, name, kind, make, branches, x0=(0.0, 0.0), exact=False, **opts):
        self.name, self.kind, self.make, self.branches = name, kind, make, set(branches)
        self.x0 = np.asarray(x0, dtype=np.float64)
        self.exact = exact                       # scripted integer data: certified as exact equality, host-callback drivers
        self.opts = dict(x_tol=1e-8, f_tol=1e-8, g_tol=1e-8, iterations=1000, delta=None, lower=None, upper=None)
        self.opts.update(opts)
        self.m, self.n = M, N

    @property
    def bounded(self):
        return self.opts["lower"] is not None or self.opts["upper"] is not None


def _s(*fs, Js=(J0,)):
    return lambda: Scripted(fs, Js)


ZERO = dict(x_tol=0.0, f_tol=0.0, g_tol=0.0)
J_ZERO_COLUMN = np.array([[0.0, 0.0], [0.0, 1.0], [0.0, 0.0], [0.0, 0.0]])
J_WIDE = np.array([[2.0 ** -12, 0.0], [0.0, 2.0 ** 60], [0.0, 0.0], [0.0, 0.0]])
J_TINY = 2.0 ** -510 * J0
J_NAN = np.array([[np.nan, 0.0], [0.0, 1.0], [0.0, 0.0], [0.0, 0.0]])


def _both(name, make, branches, lm=(), dogleg=(), lm_opts=None, dl_opts=None, x0=(0.0, 0.0), **opts):
    """One problem through both loops: LM at delta = 1 (dx = f / 2 on J0), Dogleg at delta = 64 (case 1, dx = f on J0)."""
    lo, do = dict(delta=1.0), dict(delta=64.0)
    lo.update(opts)
    do.update(opts)
    lo.update(lm_opts or {})
    do.update(dl_opts or {})
    return [Case("lm_" + name, "lm", make[0] if isinstance(make, tuple) else make, set(branches) | set(lm), x0=x0, exact=True, **lo),
            Case("dogleg_" + name, "dogleg", make[1] if isinstance(make, tuple) else make, set(branches) | set(dogleg),
                 x0=x0, exact=True, **do)]


@functools.lru_cache(maxsize=None)
def cases():
    c = []
    # ---------------------------------------------------------------------------------------------- LM, model
    c.append(Case("lm_accept_grow", "lm", Model, {"accept", "grow_q_le_third", "iterations_exhausted"}, x0=(0.1, 0.1),
                  iterations=3, **ZERO))
    c.append(Case("lm_delta_cap", "lm", Model, {"accept", "delta_cap"}, x0=(0.1, 0.1), iterations=2, delta=4e15, **ZERO))
    c.append(Case("lm_reject_to_floor", "lm", lambda: Model(lie=True),
                  {"reject", "delta_floor"} | {"decrease_factor_%d" % (2 ** k) for k in range(1, 12)}, x0=(0.1, 0.1),
                  iterations=13, delta=10.0, **ZERO))
    c.append(Case("lm_decrease_factor_reset", "lm", lambda: Model(bad=(1, 2, 4)),
                  {"reject", "accept", "decrease_factor_2", "decrease_factor_4", "decrease_factor_reset"}, x0=(0.1, 0.1),
                  iterations=4, delta=1.0, **ZERO))
    # ---------------------------------------------------------------------------------------------- LM, scripted
    c.append(Case("lm_rho_half", "lm", _s((4, 0, 0, 0), (3, 1, 0, 0)), {"accept", "grow_q_gt_third"}, exact=True, delta=1.0,
                  iterations=1))
    c.append(Case("lm_zero_residual", "lm", _s((0, 0, 0, 0)), {"pred_red_zero", "reject", "x_converged"}, exact=True,
                  delta=1.0))
    c.append(Case("lm_clamp_zero_column", "lm", _s((4, 2, 0, 0), (4, 1, 0, 0), Js=(J_ZERO_COLUMN,)),
                  {"clamp_low", "clamp_zero_column", "accept"}, exact=True, delta=1.0, iterations=1))
    # ---------------------------------------------------------------------------------------------- Dogleg, model
    c.append(Case("dogleg_case1", "dogleg", Model, {"case1", "accept", "delta_scaled_by_wnorm_x", "grow_keeps_delta"},
                  x0=(0.1, 0.1), iterations=3, delta=100.0, **ZERO))
    c.append(Case("dogleg_case2", "dogleg", Model, {"case2", "accept", "grow_3wnorm"}, x0=(0.1, 0.1), iterations=3,
                  delta=1e-3, **ZERO))
    c.append(Case("dogleg_case3", "dogleg", lambda: Model(A=A_SKEW, b=B_SKEW), {"case3", "beta_cc_positive", "accept"},
                  x0=(0.9, -0.9), iterations=4, delta=0.5, **ZERO))
    c.append(Case("dogleg_x0_zero", "dogleg", Model, {"delta_not_scaled", "accept"}, iterations=3, **ZERO))
    c.append(Case("dogleg_halve_to_floor", "dogleg", lambda: Model(lie=True), {"reject", "halve", "reuse", "delta_floor"},
                  iterations=58, delta=1.0, **ZERO))
    c.append(Case("dogleg_reuse_then_accept", "dogleg", lambda: Model(bad=(1,)), {"reject", "reuse", "accept", "halve"},
                  x0=(0.1, 0.1), iterations=3, delta=1.0, **ZERO))
    c.append(Case("dogleg_zero_gradient", "dogleg", lambda: Model(b=np.zeros(M)),
                  {"alpha_zero_gradient", "case1", "pred_red_zero", "x_converged"}, delta=1.0))
    # ---------------------------------------------------------------------------------------------- Dogleg, scripted
    c.append(Case("dogleg_rho_eq_quarter", "dogleg", _s((4, 0, 0, 0), (2, 2, 2, 0)), {"rho_eq_0.25", "delta_kept", "accept"},
                  exact=True, delta=8.0, iterations=1))
    c.append(Case("dogleg_rho_eq_three_quarters", "dogleg", _s((4, 0, 0, 0), (2, 0, 0, 0)),
                  {"rho_eq_0.75", "delta_kept", "accept"}, exact=True, delta=8.0, iterations=1))
    c.append(Case("dogleg_clamp_absolute", "dogleg", _s((1, 2.0 ** 60, 0, 0), (0, 0, 0, 0), Js=(J_WIDE,)),
                  {"clamp_low", "clamp_high", "accept", "grow_3wnorm"}, exact=True, delta=2.0 ** 54, iterations=1))
    # ---------------------------------------------------------------------------------------------- both loops, scripted
    c += _both("f_alone", _s((4, 0, 0, 0), (2, 2, 2, 0)), {"f_converged_alone", "accept"}, f_tol=0.5)
    c += _both("f_on_rejected_step", _s((4, 0, 0, 0), (0, 4, 0, 0)),
               {"f_satisfied_on_rejected", "reject", "iterations_exhausted"}, f_tol=0.5, iterations=1)
    c += _both("x_alone", _s((4, 0, 0, 0), (1, 0, 0, 0)), {"x_converged_alone", "accept"}, x_tol=10.0)
    c += _both("g_alone", _s((4, 0, 0, 0), (1, 0, 0, 0)), {"g_converged_alone", "accept"}, g_tol=10.0)
    c += _both("f_before_x", _s((4, 0, 0, 0), (2, 2, 2, 0)), {"two_satisfied", "f_converged"}, f_tol=0.5, x_tol=10.0)
    c += _both("x_before_g", _s((4, 0, 0, 0), (1, 0, 0, 0)), {"two_satisfied", "x_converged"}, x_tol=10.0, g_tol=10.0)
    c += _both("iterations_zero", _s((4, 0, 0, 0)), {"iterations_zero"}, iterations=0)
    c += _both("nonfinite_after_reject", _s((4, 2, 0, 0), (1, 1, 0, 0), Js=(J_NAN,)),
               {"reject", "nonfinite_after_reject", "nonfinite"}, iterations=3)
    c += _both("nonfinite_after_accept", _s((2.0 ** 511, 0, 0, 0), (2.0 ** 509, 0, 0, 0), Js=(J_TINY,)),
               {"accept", "nonfinite_after_accept", "nonfinite"}, x0=(-1.9 * 2.0 ** 1023, 0.0), iterations=3,
               lm_opts=dict(delta=1e6), dl_opts=dict(delta=None))
    c += _both("lower_bound", (_s((4, -2, 0, 0), (4, 1, 0, 0)), _s((4, -2, 0, 0), (4, 0, 0, 0))),
               {"proj_lower", "proj_inward_kept", "clip_lower", "accept"}, lower=np.zeros(N), iterations=1)
    c += _both("upper_bound", (_s((-4, 2, 0, 0), (-4, 1, 0, 0)), _s((-4, 2, 0, 0), (-4, 0, 0, 0))),
               {"proj_upper", "proj_inward_kept", "clip_upper", "accept"}, upper=np.zeros(N), iterations=1)
    c += _both("clip_all_zero", _s((4, 2, 0, 0)), {"clip_all_zero", "pred_red_zero", "reject", "two_satisfied", "x_converged"},
               lower=np.zeros(N))
    c += _both("x0_outside", _s((4, 0, 0, 0)), {"refused_bounds"}, lower=np.ones(N))
    out = {k.name: k for k in c}
    assert len(out) == len(c)
    return out


# Every branch the tier is asked for -> the label that certifies it; None: not reached (module docstring).
BRANCHES = {
    "lm": {"accept": "accept", "reject": "reject", "delta grown, q <= 1/3": "grow_q_le_third",
           "delta grown, q > 1/3": "grow_q_gt_third", "delta capped at MAX_DELTA": "delta_cap",
           "decrease_factor 2": "decrease_factor_2", "decrease_factor 4": "decrease_factor_4",
           "decrease_factor 8": "decrease_factor_8", "delta at the MIN_DELTA floor": "delta_floor",
           "decrease_factor reset by an accept": "decrease_factor_reset", "pred_red == 0": "pred_red_zero",
           "colsumabs2 clamped at MIN_DIAGONAL * mean": "clamp_low", "all-zero column": "clamp_zero_column",
           "colsumabs2 clamped at MAX_DIAGONAL * mean": None},
    "dogleg": {"case 1": "case1", "case 2": "case2", "case 3": "case3", "beta for cc > 0": "beta_cc_positive",
               "beta for cc <= 0": None, "delta *= wnorm(x)": "delta_scaled_by_wnorm_x", "x0 = 0: no scaling": "delta_not_scaled",
               "rho < 0.25 halves": "halve", "halved to the MIN_DELTA floor": "delta_floor",
               "rho > 0.75 grows to 3 wnorm_dx": "grow_3wnorm", "rho > 0.75 keeps delta": "grow_keeps_delta",
               "rho == 0.25 keeps delta": "rho_eq_0.25", "rho == 0.75 keeps delta": "rho_eq_0.75", "re-use after a rejection": "reuse",
               "diagonal clamped at MIN_DIAGONAL": "clamp_low", "diagonal clamped at MAX_DIAGONAL": "clamp_high",
               "alpha with a zero gradient": "alpha_zero_gradient"},
}
COMMON = {"f_converged alone": "f_converged_alone", "x_converged alone": "x_converged_alone",
          "g_converged alone": "g_converged_alone", "f satisfied on a rejected step": "f_satisfied_on_rejected",
          "two conditions at once": "two_satisfied", "iterations exhausted": "iterations_exhausted",
          "iterations = 0": "iterations_zero", "non-finite point after a rejected step": "nonfinite_after_reject",
          "non-finite point after an accepted step": "nonfinite_after_accept", "projection, active lower bound": "proj_lower",
          "projection, active upper bound": "proj_upper", "active bound, gradient inward": "proj_inward_kept",
          "clip below": "clip_lower", "clip above": "clip_upper", "clip makes dx = 0": "clip_all_zero",
          "x0 outside the bounds": "refused_bounds"}
for _k in BRANCHES:
    BRANCHES[_k].update(COMMON)


# ------------------------------------------------------------------------------------------------ runners
def twin(case, dtype=np.float64, plant=None, solver="direct"):
    p = case.make()

    def f(x):
        out = np.zeros(case.m, dtype=dtype)
        p.f(out, x)
        return out

    def g(x):
        J = np.zeros((case.m, case.n), dtype=dtype)
        p.g(J, x)
        return J

    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        r = R.optimize(case.kind, f, g, case.x0, dtype=dtype, plant=plant, solver=solver, **case.opts)
    r.f_script_calls, r.g_script_calls = p.nf, p.ng
    return r


def oracle(case, solver=None):
    from oracle import oracle as O
    p = case.make()
    m, n = case.m, case.n

    def g(jv, x):
        J = np.zeros((m, n))
        p.g(J, x)
        jv[:] = J.reshape(-1, order="F")

    o = dict(case.opts)
    delta = o.pop("delta")
    r = O.optimize(O.LM if case.kind == "lm" else O.DOGLEG, O.QR if solver is None else solver, O.Mat(dense=np.zeros((m, n))),
                   case.x0, p.f, g, delta=-1.0 if delta is None else delta, **o)
    r.f_script_calls, r.g_script_calls = p.nf, p.ng
    return r


class Certified:
    pass


@functools.lru_cache(maxsize=None)
def certify(name, solver="direct"):
    """The twin in both precisions and the oracle on one case; what the device tier compares against.  solver="lsmr": twin
    and oracle with the LSMR solve, for the drivers that iterate."""
    from oracle import oracle as O
    z = Certified()
    z.case = c = cases()[name]
    z.f64, z.ld, z.oracle = twin(c, solver=solver), twin(c, LD, solver=solver), oracle(c, O.LSMR if solver == "lsmr" else O.QR)
    z.labels = R.labels(z.f64) & R.labels(z.ld)
    z.accept = [int(rec["accepted"]) for rec in z.f64.its]
    return z


def summary(r):
    """(status, iterations, converged, x, f, g, f_calls, g_calls) of a twin Run or an oracle Result."""
    return (int(r.status), int(r.iterations), bool(r.converged), bool(r.x_converged), bool(r.f_converged),
            bool(r.g_converged), int(r.f_calls), int(r.g_calls))


# ------------------------------------------------------------------------------------------------ index spread
def _frac(j, c):
    return np.mod((j + 1.0) * c, 1.0)


class Spread:
    """The index-spread problem at one n (module docstring)."""
    offsets = (0, 1, 3)

    def __init__(self, n):
        self.n, self.m = n, n + 3
        j = np.arange(n)
        u, v = _frac(j, 0.6180339887498949), _frac(j, 0.7548776662466927)
        self.at = np.array(sorted({i for i in SPREAD_AT if i < n} | {n - 1}))
        scale = np.ones(n)
        scale[self.at] = 4.0
        self.vals = np.array([1.0, 0.5, -0.25])[None, :] * (1.0 + 0.5 * u)[:, None] * scale[:, None]
        sign = np.where(j % 2 == 0, 1.0, -1.0)
        self.x_true = sign * (0.1 + 0.3 * v)
        A = R.Band(self.vals.astype(LD), self.offsets)
        noise = 0.02 * (_frac(np.arange(self.m), 0.5698402909980532) - 0.5)       # a residual that does not vanish at the minimizer
        self.b = A.mul(np.tanh(self.x_true.astype(LD))).astype(np.float64) + noise
        self.x0 = np.zeros(n)
        self.lower, self.upper = np.full(n, -np.inf), np.full(n, np.inf)
        for i in self.at:
            if self.x_true[i] > 0:
                self.upper[i] = 0.5 * self.x_true[i]
            else:
                self.lower[i] = 0.5 * self.x_true[i]
        self.colptr = (3 * np.arange(n + 1)).astype(np.int32)
        self.rowval = (j[:, None] + np.array(self.offsets)[None, :]).reshape(-1).astype(np.int32)
        self.nzval = self.vals.reshape(-1).copy()

    @staticmethod
    def delta(kind):
        """LM: the default.  Dogleg: x0 = 0 leaves delta unscaled, and a radius of 1 over 16385 components would keep every
        component away from its bound for the whole run; 1000 admits the Gauss-Newton step."""
        return 10.0 if kind == "lm" else 1000.0

    def twin(self, kind, dtype=np.float64, bounded=True, plant=None, iterations=SPREAD_ITERATIONS):
        vals, b = self.vals.astype(dtype), self.b.astype(dtype)
        A = R.Band(vals, self.offsets)

        def f(x):
            return A.mul(np.tanh(x)) - b

        def g(x):
            t = np.tanh(x)
            return R.Band(vals * (1 - t * t)[:, None], self.offsets)

        return R.optimize(kind, f, g, self.x0, dtype=dtype, plant=plant, iterations=iterations, solver="lsmr", delta=self.delta(kind),
                          lower=self.lower if bounded else None, upper=self.upper if bounded else None, **ZERO)

    def oracle(self, kind, bounded=True, iterations=SPREAD_ITERATIONS):
        from oracle import oracle as O
        A = O.Mat(csc=(self.m, self.n, self.colptr, self.rowval, self.nzval))
        J = O.Mat(csc=(self.m, self.n, self.colptr, self.rowval, np.zeros(3 * self.n)))
        f, g, ud, keep = O.tanh_model(A, self.b)
        return O.optimize(O.LM if kind == "lm" else O.DOGLEG, O.LSMR, J, self.x0, f, g, ud=ud, iterations=iterations, delta=self.delta(kind),
                          lower=self.lower if bounded else None, upper=self.upper if bounded else None, **ZERO)


@functools.lru_cache(maxsize=None)
def spread(n):
    return Spread(n)


@functools.lru_cache(maxsize=None)
def certify_spread(n, kind, bounded=True):
    z = Certified()
    z.problem = p = spread(n)
    z.f64, z.ld, z.oracle = p.twin(kind, bounded=bounded), p.twin(kind, LD, bounded=bounded), p.oracle(kind, bounded=bounded)
    z.accept = [int(rec["accepted"]) for rec in z.f64.its]
    return z


COND_CAP = 1e6      # beyond it a comparison is one of rounding errors: it is made, and not counted as coverage


def scalar_err(v, v_hp):
    """|v - v_hp| / |v_hp| in longdouble (|v| where v_hp = 0; 0 / inf for equal / unequal non-finite values)."""
    v, v_hp = LD(v), LD(v_hp)
    if np.isnan(v_hp) or np.isinf(v_hp):
        return 0.0 if (np.isnan(v) and np.isnan(v_hp)) or v == v_hp else np.inf
    return float(abs(v - v_hp) / abs(v_hp)) if v_hp != 0 else float(abs(v))


def conditions(r64, rld):
    """Condition numbers of an iteration's continuous values with respect to the sums they are made of, from the longdouble
    record: rho = (ssr - trial_ssr) / pred_red is a quotient of differences of sums of squares (ssr / pred_red); the gradient
    norm is a maximum of sums that cancel as the fit converges (max |J|'|f| / max |J'f|); delta inherits rho's only where it
    is computed from rho (LM's growth with q > 1/3) -- a halved, kept, divided or 3 wnorm(dx) delta does not."""
    pr, gr = float(rld["pred_red"]), float(rld["maxabs_gr"])
    c_rho = float(rld["ssr_before"]) / pr if pr > 0 and np.isfinite(pr) else 1.0
    c_g = float(rld["g_terms"]) / gr if gr > 0 and np.isfinite(gr) else 1.0
    c_delta = c_rho if "grow_q_gt_third" in r64["labels"] else 1.0
    return dict(rho=max(1.0, c_rho), ssr=1.0, gnorm=max(1.0, c_g), delta=max(1.0, c_delta))


def trajectory_pieces(f64, ld, oracle_trace, kdim):
    """What the device tier compares of a certified run, iteration by iteration: (i, name, value of the longdouble twin, cond,
    bound) with bound = accuracy_common.trajectory_bound(e_ref, kdim, i + 1, cond), e_ref the float64 oracle's distance from
    the longdouble twin.  tests/test_v_gpu_trust_region.py holds the device to it, tests/test_trust_region_host.py a twin with
    an error planted."""
    import accuracy_common as ac
    out = []
    for i, (r64, rld) in enumerate(zip(f64.its, ld.its)):
        cond = conditions(r64, rld)
        for name, key in (("rho", "rho"), ("ssr", "ssr"), ("gnorm", "maxabs_gr"), ("delta", "delta")):
            hp = rld[key]
            e_ref = scalar_err(oracle_trace[name][i], hp)
            out.append((i, name, hp, cond[name], ac.trajectory_bound(e_ref, kdim, i + 1, cond[name])))
        if np.all(np.isfinite(np.asarray(rld["x"], dtype=np.float64))):
            e_ref = rel_err(oracle_trace["x"][i], rld["x"])
            out.append((i, "x", rld["x"], 1.0, ac.trajectory_bound(e_ref, kdim, i + 1)))
    return out


def piece_err(name, value, hp):
    return rel_err(value, hp) if name == "x" else scalar_err(value, hp)


def rel_err(x, x_hp):
    """||x - x_hp|| / ||x_hp|| in longdouble (|x - x_hp| where x_hp = 0)."""
    d = np.sqrt(np.sum((np.asarray(x, dtype=LD) - x_hp) ** 2))
    s = np.sqrt(np.sum(np.asarray(x_hp, dtype=LD) ** 2))
    return float(d / s) if s > 0 else float(d)
