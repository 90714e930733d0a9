"""The twin of the two outer loops: a numpy restatement of levenberg_marquardt.jl:39-144 and dogleg.jl:41-203 (with
utils.jl:7-55 and the constants of types.jl:107-111) written from the reference's text, runnable in float64 and in
numpy.longdouble.  The linear solves are direct: Householder QR on a dense Jacobian, the banded normal equations (refined in
the working precision) on a Band Jacobian; solver="lsmr" takes the reference's LSMR solve instead (tests/lsmr_reference.py),
which is what a trajectory on a driver that iterates has to be compared with.  tests/trust_region_cases.py builds the cases, tests/test_trust_region_host.py
certifies them, tests/test_v_gpu_trust_region.py holds the device loops to the certified values.

The problem is a black box: f(x) -> residual, g(x) -> Jacobian (a dense array or a Band), both in the dtype of x.

Per outer iteration the record holds every quantity a branch looks at (rho, pred_red, delta before / after, maxabs_dx,
maxabs_gr, wnorm_dgn, wnorm_dgr * alpha, cc; ssr_before and g_terms = max |J|'|f| size the rounding error of rho and of the
gradient), the clamped diagonal with the entries clamped low / high, the components the
projection zeroed and the clip changed, the `margins` (name -> (value, threshold): every comparison that decided a branch), `pure_delta` / `pure_op` where the new
delta is a pure function of the branch and the old delta (pure_delta()), and
the `labels` of the branches taken.

`plant` names a deliberate error (tests/test_trust_region_host.py: the planted errors); None is the reference.
"""
import numpy as np
import scipy.linalg as sla

import lsmr_reference

LD = np.longdouble
MIN_DELTA, MAX_DELTA = 1e-16, 1e16          # types.jl:107-108
MIN_STEP_QUALITY = 1e-3                     # types.jl:109
MIN_DIAGONAL, MAX_DIAGONAL = 1e-6, 1e32     # types.jl:110-111
DECREASE_THRESHOLD, INCREASE_THRESHOLD = 0.25, 0.75     # dogleg.jl:38-39
OK, ENONFINITE, EBOUNDS = 0, 4, 5           # as oracle.oracle numbers them
PLANTS = ("projection_skipped_from_1024", "dogleg_strictness_swapped", "decrease_factor_not_reset",
          "f_converged_on_rejected_step", "dogleg_clamp_relative")


class _BandT:
    def __init__(self, B):
        self.B = B

    def __matmul__(self, y):
        return self.B.mulT(y)


class Band:
    """Column j holds vals[j, k] at row j + offsets[k]: m = n + offsets[-1]."""

    def __init__(self, vals, offsets):
        self.vals, self.offsets = vals, tuple(offsets)
        self.n = vals.shape[0]
        self.m = self.n + self.offsets[-1]

    @property
    def shape(self):
        return self.m, self.n

    @property
    def T(self):
        return _BandT(self)

    def __matmul__(self, x):
        return self.mul(x)

    def mul(self, x):
        y = np.zeros(self.m, dtype=self.vals.dtype)
        for k, o in enumerate(self.offsets):
            y[o:o + self.n] += self.vals[:, k] * x
        return y

    def mulT(self, y):
        x = np.zeros(self.n, dtype=self.vals.dtype)
        for k, o in enumerate(self.offsets):
            x += self.vals[:, k] * y[o:o + self.n]
        return x

    def colsumabs2(self):
        return np.sum(self.vals * self.vals, axis=1)

    def gram_banded(self, diag):
        """Upper banded storage of J'J + diag(diag) for scipy.linalg.solveh_banded, in float64."""
        n, w = self.n, self.offsets[-1]
        v = self.vals.astype(np.float64)
        ab = np.zeros((w + 1, n))
        for a, oa in enumerate(self.offsets):
            for b, ob in enumerate(self.offsets):
                d = oa - ob                  # column j (entry a) and column j + d (entry b) share row j + oa
                if d < 0 or d >= n:
                    continue
                ab[w - d, d:] += v[:n - d, a] * v[d:, b]
        ab[w] += np.asarray(diag, dtype=np.float64)
        return ab


def _householder_lstsq(A, b):
    """min ||A x - b||_2 by Householder QR in the dtype of A (full column rank)."""
    A, b = A.copy(), b.copy()
    m, n = A.shape
    for k in range(n):
        v = A[k:, k].copy()
        nv = np.sqrt(np.sum(v * v))
        if nv == 0:
            continue
        v[0] += nv if v[0] >= 0 else -nv
        v /= np.sqrt(np.sum(v * v))
        A[k:, k:] -= 2 * np.outer(v, v @ A[k:, k:])
        b[k:] -= 2 * v * (v @ b[k:])
    x = np.zeros(n, dtype=A.dtype)
    for k in range(n - 1, -1, -1):
        x[k] = (b[k] - A[k, k + 1:n] @ x[k + 1:]) / A[k, k]
    return x


def solve(J, f, damp=None, solver="direct"):
    """argmin ||J x - f||^2 + x' diag(damp) x  (damp None: the Gauss-Newton step); returns (x, mul count).  solver="lsmr":
    the reference's LSMR solve with its fixed tolerances (tests/lsmr_reference.py), for the drivers that iterate."""
    T = f.dtype.type
    if solver == "lsmr":
        rec = lsmr_reference.ldiv_lsmr(J, f, damp, dtype=T)
        return rec.x, rec.nmul
    return _direct(J, f, damp), 0


def _direct(J, f, damp):
    T = f.dtype.type
    if isinstance(J, Band):
        d = np.zeros(J.n, dtype=f.dtype) if damp is None else damp
        ab = J.gram_banded(d)
        x = np.zeros(J.n, dtype=f.dtype)
        for _ in range(4 if T is LD else 2):     # refinement in the working precision against the fp64 banded factor
            r = J.mulT(f - J.mul(x)) - d * x
            x = x + sla.solveh_banded(ab, r.astype(np.float64)).astype(f.dtype)
        return x
    m, n = J.shape
    if damp is None:
        return _householder_lstsq(J, f)
    A = np.vstack([J, np.diag(np.sqrt(damp))])
    return _householder_lstsq(A, np.concatenate([f, np.zeros(n, dtype=f.dtype)]))


def _ops(J):
    if isinstance(J, Band):
        return J.colsumabs2(), J.mul, J.mulT
    return np.sum(J * J, axis=0), (lambda x: J @ x), (lambda y: J.T @ y)


def _abs_mulT(J, f):
    """|J|'|f|: the size of the terms that J'f adds up (how much of the gradient is cancellation)."""
    if isinstance(J, Band):
        return Band(np.abs(J.vals), J.offsets).mulT(np.abs(f))
    return np.abs(J).T @ np.abs(f)


def _in_float64_range(x):
    """x lives in float64 in the reference: where x - dx overflows there it is +-inf, in the longdouble run too."""
    big = np.finfo(np.float64).max
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(x) > big, np.sign(x) * np.inf, x).astype(x.dtype)


def _wdot(x, y, w):
    return np.sum(w * x * y)


def _projected(gr, x, lower, upper, rec, plant):
    """utils.jl:39-55; records which components were zeroed."""
    g = gr.copy()
    zeroed = np.zeros(len(g), dtype=bool)
    if lower is not None:
        zeroed |= (x <= lower) & (g > 0)
    if upper is not None:
        zeroed |= (x >= upper) & (g < 0) & ~zeroed
    if plant == "projection_skipped_from_1024":
        zeroed[1024:] = False
    at = np.zeros(len(g), dtype=bool)
    if lower is not None:
        at |= x <= lower
    if upper is not None:
        at |= x >= upper
    rec["zeroed"] = np.flatnonzero(zeroed)
    rec["at_bound_kept"] = np.flatnonzero(at & ~zeroed & (g != 0))
    rec["maxabs_g_raw"] = np.max(np.abs(g))
    g[zeroed] = 0
    if lower is not None and np.any(zeroed & (x <= lower)):
        rec["labels"].append("proj_lower")
    if upper is not None and np.any(zeroed & (x >= upper) & ~(False if lower is None else (x <= lower))):
        rec["labels"].append("proj_upper")
    if len(rec["at_bound_kept"]):
        rec["labels"].append("proj_inward_kept")
    return np.max(np.abs(g))


def _clip(dx, x, lower, upper, rec):
    """levenberg_marquardt.jl:89-98 / dogleg.jl:148-157: the step is clipped (Julia's min / max propagate NaN)."""
    before = dx.copy()
    if lower is not None:
        a = x - lower
        lo = np.where(np.isnan(dx) | np.isnan(a), dx + a, np.minimum(dx, a))
        if np.any(lo != dx):
            rec["labels"].append("clip_lower")
        dx = lo
    if upper is not None:
        a = x - upper
        hi = np.where(np.isnan(dx) | np.isnan(a), dx + a, np.maximum(dx, a))
        if np.any(hi != dx):
            rec["labels"].append("clip_upper")
        dx = hi
    rec["clipped"] = np.flatnonzero(before != dx)
    if len(rec["clipped"]) and not np.any(dx):
        rec["labels"].append("clip_all_zero")
    return dx


def _assess(dx, maxabs_gr, ssr, trial_ssr, x_tol, f_tol, g_tol, accepted, rec, plant):
    """utils.jl:7-31"""
    f_ok = abs(trial_ssr - ssr) <= f_tol * (abs(ssr) + f_tol)
    x_ok = np.max(np.abs(dx)) <= x_tol
    g_ok = maxabs_gr <= g_tol
    rec["satisfied"] = (bool(f_ok), bool(x_ok), bool(g_ok))
    if accepted:                          # (on a rejected step the comparison decides nothing)
        rec["margins"]["f_tol"] = (abs(trial_ssr - ssr), f_tol * (abs(ssr) + f_tol))
    rec["margins"]["x_tol"] = (np.max(np.abs(dx)), x_tol)
    rec["margins"]["g_tol"] = (maxabs_gr, g_tol)
    xc = fc = gc = False
    if (accepted or plant == "f_converged_on_rejected_step") and f_ok:
        fc = True
    elif x_ok:
        xc = True
    elif g_ok:
        gc = True
    if f_ok and not accepted:
        rec["labels"].append("f_satisfied_on_rejected")
    n_ok = int(f_ok and accepted) + int(x_ok) + int(g_ok)
    if n_ok >= 2:
        rec["labels"].append("two_satisfied")
    for flag, name in ((fc, "f_converged"), (xc, "x_converged"), (gc, "g_converged")):
        if flag:
            rec["labels"].append(name + ("_alone" if n_ok == 1 else ""))
    return xc, fc, gc


class Run:
    pass


def optimize(kind, f, g, x0, dtype=np.float64, lower=None, upper=None, delta=None, x_tol=1e-8, f_tol=1e-8, g_tol=1e-8,
             iterations=1000, plant=None, solver="direct"):
    """kind: "lm" or "dogleg".  Returns a Run: status, iterations, converged, x/f/g_converged, f_calls, g_calls, ssr, x, its."""
    assert plant is None or plant in PLANTS
    T = np.dtype(dtype).type
    x = np.asarray(x0, dtype=dtype).copy()
    lower = None if lower is None else np.asarray(lower, dtype=dtype)
    upper = None if upper is None else np.asarray(upper, dtype=dtype)
    R = Run()
    R.kind, R.its, R.status, R.bad_index = kind, [], OK, -1
    R.iterations = R.f_calls = R.g_calls = 0
    R.converged = R.x_converged = R.f_converged = R.g_converged = False
    R.x, R.ssr = x, None
    if (lower is not None and not np.all(x >= lower)) or (upper is not None and not np.all(x <= upper)):
        R.status = EBOUNDS
        return R
    lm = kind == "lm"
    delta = T(delta if delta is not None else (10.0 if lm else 1.0))
    third = T(1.0) / T(3.0) if T is LD else 1.0 / 3.0
    decrease_factor = T(2.0)
    fcur = f(x)
    R.f_calls += 1
    ssr = np.sum(fcur * fcur)
    maxabs_gr = T(np.inf)
    need_jacobian, reuse = True, False
    J = dtd = dgr = dgn = None
    wnorm_dgn = wnorm_dgr = alpha = g_terms = T(0)
    it = 0
    xc = fc = gc = False
    while not (xc or fc or gc) and it < iterations:
        it += 1
        if not np.all(np.isfinite(x)):
            R.status, R.bad_index = ENONFINITE, int(np.flatnonzero(~np.isfinite(x))[0])
            it -= 1
            break
        rec = dict(labels=[], margins={}, delta_before=delta, pure_delta=False, inner=0, ssr_before=ssr)
        if lm:
            if need_jacobian:
                J = g(x)
                R.g_calls += 1
                need_jacobian = False
            cs, mul, mulT = _ops(J)
            mean = np.sum(cs) / len(cs)
            lo, hi = T(MIN_DIAGONAL) * mean, T(MAX_DIAGONAL) * mean
            dtd = np.clip(cs, lo, hi)
            rec["clamped_low"], rec["clamped_high"] = np.flatnonzero(cs < lo), np.flatnonzero(cs > hi)
            rec["dtd"] = dtd.copy()
            if len(rec["clamped_low"]):
                rec["labels"].append("clamp_low")
                if np.any(cs == 0):
                    rec["labels"].append("clamp_zero_column")
            if len(rec["clamped_high"]):
                rec["labels"].append("clamp_high")
            rec["margins"]["clamp"] = (cs.copy(), lo, hi)
            dx, rec["inner"] = solve(J, fcur, dtd * (1 / delta), solver)
            dx = _clip(dx, x, lower, upper, rec)
            maxabs_gr = _projected(mulT(fcur), x, lower, upper, rec, plant)
            rec["g_terms"] = np.max(_abs_mulT(J, fcur))
        else:
            if not reuse:
                J = g(x)
                R.g_calls += 1
                cs, mul, mulT = _ops(J)
                if plant == "dogleg_clamp_relative":
                    mean = np.sum(cs) / len(cs)
                    lo, hi = T(MIN_DIAGONAL) * mean, T(MAX_DIAGONAL) * mean
                else:
                    lo, hi = T(MIN_DIAGONAL), T(MAX_DIAGONAL)
                dtd = np.clip(cs, lo, hi)
                rec["clamped_low"], rec["clamped_high"] = np.flatnonzero(cs < lo), np.flatnonzero(cs > hi)
                rec["dtd"] = dtd.copy()
                if len(rec["clamped_low"]):
                    rec["labels"].append("clamp_low")
                if len(rec["clamped_high"]):
                    rec["labels"].append("clamp_high")
                rec["margins"]["clamp"] = (cs.copy(), lo, hi)
                if it == 1:
                    wx = np.sqrt(_wdot(x, x, dtd))
                    if wx > 0:
                        delta = delta * wx
                        rec["labels"].append("delta_scaled_by_wnorm_x")
                    else:
                        rec["labels"].append("delta_not_scaled")
                    rec["delta_before"] = delta
                dgr = mulT(fcur)
                maxabs_gr = _projected(dgr, x, lower, upper, rec, plant)
                g_terms = np.max(_abs_mulT(J, fcur))
                dgr = dgr / dtd
                wnorm_dgr = np.sqrt(_wdot(dgr, dgr, dtd))
                jg = mul(dgr)
                with np.errstate(invalid="ignore", divide="ignore"):
                    alpha = wnorm_dgr * wnorm_dgr / np.sum(jg * jg)
                if wnorm_dgr == 0:
                    rec["labels"].append("alpha_zero_gradient")
                dgn, rec["inner"] = solve(J, fcur, None, solver)
                wnorm_dgn = np.sqrt(_wdot(dgn, dgn, dtd))
            else:
                rec["labels"].append("reuse")
            rec["wnorm_dgn"], rec["cauchy"], rec["g_terms"] = wnorm_dgn, wnorm_dgr * alpha, g_terms
            rec["margins"]["case1"] = (wnorm_dgn, delta)
            if wnorm_dgn <= delta:
                rec["labels"].append("case1")
                dx, wnorm_dx = dgn.copy(), wnorm_dgn
            elif wnorm_dgr * alpha >= delta:
                rec["margins"]["case2"] = (wnorm_dgr * alpha, delta)
                rec["labels"].append("case2")
                dx, wnorm_dx = dgr * (delta / wnorm_dgr), delta
            else:
                rec["margins"]["case2"] = (wnorm_dgr * alpha, delta)
                rec["labels"].append("case3")
                b_dot_a = alpha * _wdot(dgr, dgn, dtd)
                a2 = (alpha * wnorm_dgr) ** 2
                bma2 = a2 - 2 * b_dot_a + wnorm_dgn ** 2
                cc = b_dot_a - a2
                d = np.sqrt(cc * cc + bma2 * (delta * delta - a2))
                rec["cc"] = cc
                rec["margins"]["cc"] = (cc, a2)
                if cc <= 0:
                    beta = (d - cc) / bma2
                    rec["labels"].append("beta_cc_nonpositive")
                else:
                    beta = (delta * delta - a2) / (d + cc)
                    rec["labels"].append("beta_cc_positive")
                dx = dgn * beta + (alpha * (1 - beta)) * dgr
                wnorm_dx = np.sqrt(_wdot(dx, dx, dtd))
            dx = _clip(dx, x, lower, upper, rec)
            _, mul, mulT = _ops(J)
        x = _in_float64_range(x - dx)
        ftrial = f(x)
        R.f_calls += 1
        trial_ssr = np.sum(ftrial * ftrial)
        fpred = mul(dx) - fcur
        pred_red = abs(ssr - np.sum(fpred * fpred))
        with np.errstate(invalid="ignore", over="ignore"):
            rho = (ssr - trial_ssr) / pred_red if pred_red > 0 else T(0)
        if not pred_red > 0:
            rec["labels"].append("pred_red_zero")
        msq = T(MIN_STEP_QUALITY)
        if lm:
            accepted = bool(rho > msq)
        elif plant == "dogleg_strictness_swapped":
            accepted = bool(rho > msq)
        else:
            accepted = bool(rho >= msq)
        rec["margins"]["accept"] = (rho, msq)
        rec["rho"], rec["pred_red"], rec["accepted"] = rho, pred_red, accepted
        rec["maxabs_dx"], rec["maxabs_gr"] = np.max(np.abs(dx)), maxabs_gr
        rec["labels"].append("accept" if accepted else "reject")
        xc, fc, gc = _assess(dx, maxabs_gr, ssr, trial_ssr, x_tol, f_tol, g_tol, accepted, rec, plant)
        if accepted:
            fcur, ssr = ftrial, trial_ssr
            if not np.all(np.isfinite(x)):
                rec["labels"].append("nonfinite_after_accept")
        else:
            x = x + dx
            if not np.all(np.isfinite(x)):
                rec["labels"].append("nonfinite_after_reject")
        if lm:
            if accepted:
                q = 1 - (2 * rho - 1) ** 3
                rec["margins"]["q"] = (q, third)
                grown = delta / max(third, q)
                rec["labels"].append("grow_q_le_third" if q <= third else "grow_q_gt_third")
                rec["pure_delta"], rec["pure_op"] = bool(q <= third), ("third",)
                rec["margins"]["cap"] = (grown, T(MAX_DELTA))
                if grown >= T(MAX_DELTA):
                    rec["labels"].append("delta_cap")
                    rec["pure_delta"], rec["pure_op"] = True, ("cap",)
                delta = min(grown, T(MAX_DELTA))
                if decrease_factor != 2:
                    rec["labels"].append("decrease_factor_reset")
                if plant != "decrease_factor_not_reset":
                    decrease_factor = T(2.0)
                need_jacobian = True
            else:
                rec["labels"].append("decrease_factor_%d" % int(decrease_factor))
                shrunk = delta / decrease_factor
                rec["margins"]["floor"] = (shrunk, T(MIN_DELTA))
                if shrunk <= T(MIN_DELTA):
                    rec["labels"].append("delta_floor")
                delta = max(shrunk, T(MIN_DELTA))
                rec["pure_delta"], rec["pure_op"] = True, ("divide", float(decrease_factor))
                decrease_factor = decrease_factor * 2
        else:
            reuse = not accepted
            strict = plant != "dogleg_strictness_swapped"
            rec["margins"]["decrease"] = (rho, T(DECREASE_THRESHOLD))
            rec["margins"]["increase"] = (rho, T(INCREASE_THRESHOLD))
            if (rho < DECREASE_THRESHOLD) if strict else (rho <= DECREASE_THRESHOLD):
                rec["margins"]["floor"] = (delta * T(0.5), T(MIN_DELTA))
                if delta * T(0.5) <= T(MIN_DELTA):
                    rec["labels"].append("delta_floor")
                delta = max(T(MIN_DELTA), delta * T(0.5))
                rec["labels"].append("halve")
                rec["pure_delta"], rec["pure_op"] = True, ("halve",)
            elif (rho > INCREASE_THRESHOLD) if strict else (rho >= INCREASE_THRESHOLD):
                rec["margins"]["grow"] = (3 * wnorm_dx, delta)
                rec["labels"].append("grow_3wnorm" if 3 * wnorm_dx > delta else "grow_keeps_delta")
                rec["pure_delta"], rec["pure_op"] = not 3 * wnorm_dx > delta, ("keep",)
                delta = max(delta, 3 * wnorm_dx)
            else:
                rec["labels"].append("delta_kept")
                if rho == DECREASE_THRESHOLD:
                    rec["labels"].append("rho_eq_0.25")
                if rho == INCREASE_THRESHOLD:
                    rec["labels"].append("rho_eq_0.75")
                rec["pure_delta"], rec["pure_op"] = True, ("keep",)
        rec["delta"], rec["ssr"], rec["x"] = delta, ssr, x.copy()
        R.its.append(rec)
    R.iterations = it
    R.x_converged, R.f_converged, R.g_converged = xc, fc, gc
    R.converged = xc or fc or gc
    R.x, R.ssr = x, ssr
    if R.status == OK and not R.converged:
        R.its and R.its[-1]["labels"].append("iterations_exhausted")
    return R


def pure_delta(op, before):
    """delta after an iteration whose update is a pure function of the branch taken (rec["pure_op"]), from delta before it,
    in float64 as the reference computes it."""
    before = float(before)
    if op[0] == "third":
        return min(before / (1.0 / 3.0), MAX_DELTA)
    if op[0] == "cap":
        return MAX_DELTA
    if op[0] == "divide":
        return max(before / op[1], MIN_DELTA)
    if op[0] == "halve":
        return max(MIN_DELTA, before * 0.5)
    assert op[0] == "keep"
    return before


def labels(R):
    out = set()
    for rec in R.its:
        out.update(rec["labels"])
    if R.iterations == 0 and R.status == OK:
        out.add("iterations_zero")
    if R.status == EBOUNDS:
        out.add("refused_bounds")
    if R.status == ENONFINITE:
        out.add("nonfinite")
    return out
