"""Robust loss tier, shared part (tests/test_robust_loss_host.py, tests/test_x_gpu_robust_loss.py): the cases, the longdouble
reference of the transform and the independent gradient of the robust cost.  Nothing here touches a device.

Cases (each: raw f_ / g_ on the host containers of lsq_amd, a start, sigmas over three decades, the planted outlier rows):
    decay    dense 40 x 3 exponential decay a exp(-k t) + d, four rows displaced by +50
    line     plain CSC 300 x 40, r = A x - b, ragged pattern (column 1 empty, column 2 full), 30 displaced rows.  Linear in x:
             with huber / soft_l1 the cost is convex, so a stationary point is the global minimiser -- the gradient test certifies
             the result without a second optimiser
    blocks   BlockDiagonal B = 5, mb = 12, nb = 3, a decay per block; block 1 has two outliers, block 3 every row displaced
    global   BorderedBlockDiagonal B = 4, mb = 10, nb = 2, ng = 3: a_b exp(-k t) + d_b + s1 sin(3t) + s2 cos(3t), (k, s1, s2) shared

The reference of the transform is c sqrt(rho) and rho' sqrt(s) / sqrt(rho) in numpy.longdouble, written in forms without
cancellation (soft_l1: rho = 2 s / (sqrt(1 + s) + 1)).  The metric is the largest relative error over the elements (an exact 0
must be 0, a non-finite element must keep its class); the rule is accuracy_common.bound(e_ref, 1).  On the host the twin itself
is judged, so e_ref = 0: the bound is the rule's floor, 16 * 16 * 2^-53 -- a handful of roundings, from the number format.  On
the device e_ref is the twin's own error on the same inputs."""
import numpy as np
import scipy.sparse as sp

import accuracy_common as ac
import lsq_amd as lsq

LD = np.longdouble
LOSSES = ("linear", "huber", "soft_l1", "cauchy")
BITWISE = ("linear", "huber", "soft_l1")


# ------------------------------------------------------------------------------------------------ the transform's reference
def transform_inputs(c):
    """The special inputs of the tier, as raw residuals for scale c (no sigma), plus a log grid for the monotonicity check."""
    pm = lambda v: [v, -v]     # noqa: E731
    special = [0.0, -0.0] + pm(1e-200) + pm(2.0 ** -28 * c) + pm(c) + pm(np.nextafter(c, np.inf)) + pm(np.nextafter(c, -np.inf)) \
        + pm(3.0 * c) + pm(1e200) + [np.nan, np.inf, -np.inf]
    return np.array(special)


def grid_inputs(c, count=400):
    g = c * np.logspace(-12, 12, count)
    return np.concatenate([g, -g])


def extreme_inputs(c):
    """The top of the range, for runs without sigmas (dividing by a small sigma would overflow z itself): a = 1e308 / max(c, 1)
    is where 2a overflows (huber) and where 1 / a^2 has long underflowed (cauchy)."""
    v = 1e308 * min(c, 1.0)
    return np.array([v, -v, 0.5 * v, -0.5 * v])


def reference(f, loss, c, sigma=None):
    """(rt, w, rho) in longdouble for finite f."""
    z = f.astype(LD) / (LD(1) if sigma is None else sigma.astype(LD))
    cc = LD(c)
    a = np.abs(z) / cc
    s = a * a
    one = LD(1)
    if loss == "linear":
        rho, d = s, np.ones_like(s)
    elif loss == "huber":
        big = a > 1
        rho = np.where(big, 2 * a - 1, s)
        d = np.where(big, one / np.where(big, a, one), one)
    elif loss == "soft_l1":
        t = np.sqrt(1 + s)
        rho, d = 2 * s / (t + 1), one / t
    else:
        rho, d = np.log1p(s), one / (1 + s)
    nz = s > 0
    w = np.where(nz, d * a / np.sqrt(np.where(nz, rho, one)), one)
    return np.copysign(cc * np.sqrt(rho), z), w, rho


def rel_err(got, ref):
    """max |got - ref| / |ref| in longdouble over finite references; where ref is 0 got must be 0 with the same sign."""
    got, ref = np.asarray(got), np.asarray(ref)
    zero = ref == 0
    if np.any(got[zero] != 0) or np.any(np.signbit(got[zero]) != np.signbit(ref[zero])) or not np.all(np.isfinite(got)):
        return np.inf
    if np.all(zero):
        return 0.0
    return float(np.max(np.abs(got[~zero].astype(LD) - ref[~zero]) / np.abs(ref[~zero])))


def transform_errors(rt, rowf, f, loss, c, sigma=None):
    """(e_rt, e_w, e_sq) of a candidate (rt, rowfactor) on the finite elements of f: against c sqrt(rho), against the analytic
    derivative (rowfactor times sigma is w), and rt^2 against c^2 rho."""
    fin = np.isfinite(f)
    sg = None if sigma is None else sigma[fin]
    rt_ref, w_ref, rho = reference(f[fin], loss, c, sg)
    w_got = rowf[fin].astype(LD) * (LD(1) if sg is None else sg.astype(LD))
    sq = rt[fin].astype(LD) ** 2
    return rel_err(rt[fin], rt_ref), rel_err(w_got, w_ref), rel_err(sq, LD(c) ** 2 * rho)


def nonfinite_classes_kept(rt, f):
    bad = ~np.isfinite(f)
    return bool(np.array_equal(np.isnan(rt[bad]), np.isnan(f[bad])) and np.array_equal(rt[bad][np.isinf(f[bad])], f[bad][np.isinf(f[bad])])
                and np.all(np.isfinite(rt[~bad])))


# ------------------------------------------------------------------------------------------------ the independent gradient
def rho_prime(s, loss):
    if loss == "linear":
        return np.ones_like(s)
    if loss == "huber":
        return np.where(s > 1, 1.0 / np.sqrt(np.where(s > 1, s, 1.0)), 1.0)
    if loss == "soft_l1":
        return 1.0 / np.sqrt(1.0 + s)
    return 1.0 / (1.0 + s)


def robust_gradient(case, x, loss, c, sigma):
    """J'(rho' f / sigma^2) at x from the RAW f_ and g_ (the exact gradient of c^2 / 2 sum(rho)), its infinity norm and the
    accuracy_common.product_bound of that product (K: stored entries per column, c = 3 further roundings: rho' f, / sigma^2
    and the device's own gradient being formed from rounded J~ and r~ instead)."""
    f = np.zeros(case.m)
    case.f_(f, x)
    J = case.new_J()
    case.g_(J, x)
    sg = np.ones(case.m) if sigma is None else sigma
    v = rho_prime((f / (sg * c)) ** 2, loss) * f / sg ** 2
    S = sp.csc_matrix(J) if isinstance(J, np.ndarray) else J.tocsc()
    grad = S.T @ v
    mag = abs(S).T @ np.abs(v)
    K = np.diff(S.indptr)
    return grad, float(np.max(np.abs(grad))), np.asarray(ac.product_bound(K, 3, mag), dtype=np.float64)


# ------------------------------------------------------------------------------------------------ the cases
class Case:
    def __init__(self, name, kind, m, n, x0, f_, g_, new_J, outliers, seed):
        self.name, self.kind, self.m, self.n, self.x0 = name, kind, m, n, x0
        self.f_, self.g_, self.new_J, self.outliers = f_, g_, new_J, np.asarray(outliers)
        rng = np.random.default_rng(seed)
        self.sigma = 10.0 ** rng.uniform(-1.5, 1.5, m)         # three decades

    def problem(self, f_=None, g_="raw", x0=None):
        """A LeastSquaresProblem on fresh containers; g_ = None leaves the Jacobian to central differences (on the device for
        the block containers and, by colours, for the sparse pattern)."""
        g_ = self.g_ if isinstance(g_, str) else g_
        autodiff = "central_coloured" if (g_ is None and self.kind == "csc") else "central"
        return lsq.LeastSquaresProblem(x=(self.x0 if x0 is None else x0).copy(), y=np.zeros(self.m), f_=f_ or self.f_, g_=g_,
                                       J=self.new_J(), autodiff=autodiff)

    def twin_problem(self, loss, f_scale, sigma, fd=False, x0=None):
        rf, rg = lsq.robust_twin(self.f_, None if fd else self.g_, loss, f_scale, sigma)
        return self.problem(rf, rg, x0)


def _decay_model(t, a, k, d):
    return a * np.exp(-k * t) + d


def decay_case():
    m, rng = 40, np.random.default_rng(101)
    t = np.linspace(0.0, 4.0, m)
    data = _decay_model(t, 5.0, 1.3, 0.5) + 0.05 * rng.standard_normal(m)
    out = np.array([3, 11, 22, 35])
    data[out] += 50.0

    def f_(o, x):
        o[:] = _decay_model(t, x[0], x[1], x[2]) - data

    def g_(J, x):
        e = np.exp(-x[1] * t)
        J[:, 0] = e
        J[:, 1] = -x[0] * t * e
        J[:, 2] = 1.0

    return Case("decay", "dense", m, 3, np.array([3.0, 0.8, 0.0]), f_, g_, lambda: np.zeros((m, 3), order="F"), out, 102)


def line_pattern():
    m, n = 300, 40
    rng = np.random.default_rng(111)
    S = sp.random(m, n, density=0.08, format="lil", random_state=rng, data_rvs=rng.standard_normal)
    S[:, 1] = 0                                     # an empty column
    S[:, 2] = rng.standard_normal(m).reshape(-1, 1)  # a full one
    S = S.tocsc()
    S.eliminate_zeros()
    S.sort_indices()
    return S


def line_case(dense=False):
    A = line_pattern()
    m, n = A.shape
    rng = np.random.default_rng(112)
    xt = rng.uniform(-1.0, 1.0, n)
    sigma = 10.0 ** np.random.default_rng(113).uniform(-1.5, 1.5, m)       # (the Case's own sigmas: same seed)
    b = A @ xt + 0.2 * sigma * rng.standard_normal(m)                      # noise of 0.2 sigma: |z| stays far below a scale of 2
    # displaced by 20 .. 60 sigma, among the less precise half of the rows: a displaced row whose weight dwarfs its neighbours'
    # is a leverage point, which no loss of this family can tell from good data
    out = np.sort(rng.choice(np.flatnonzero(sigma >= np.median(sigma)), size=30, replace=False))
    b[out] += rng.choice([-1.0, 1.0], 30) * rng.uniform(20.0, 60.0, 30) * sigma[out]
    R = A.tocsr()
    vals = A.data.copy()

    def f_(o, x):
        o[:] = R @ x - b

    def g_(J, x):
        J.data[:] = vals

    def new_J():
        return sp.csc_matrix((np.zeros(A.nnz), A.indices.copy(), A.indptr.copy()), shape=A.shape)

    if dense:       # the same problem with the Jacobian stored densely: QR() takes the empty column (minimum norm)
        D = A.toarray()

        def g_(J, x):       # noqa: F811
            J[:, :] = D

        new_J = lambda: np.zeros((m, n), order="F")     # noqa: E731
    c = Case("line dense" if dense else "line", "dense" if dense else "csc", m, n, np.zeros(n), f_, g_, new_J, out, 113)
    c.A, c.b = A, b
    return c


def blocks_case(copies=1, single=False):
    """copies > 1: the five blocks tiled that many times (optimize_batched_ on 300 copies: the same fits, many of them);
    single: block 1 alone (B = 1)."""
    B0, mb, nb = 5, 12, 3
    rng = np.random.default_rng(121)
    t = np.linspace(0.0, 3.0, mb)
    truth = np.column_stack([rng.uniform(3.0, 6.0, B0), rng.uniform(0.8, 1.6, B0), rng.uniform(-0.5, 0.5, B0)])
    data = np.stack([_decay_model(t, *truth[b]) for b in range(B0)]) + 0.03 * rng.standard_normal((B0, mb))
    planted = np.zeros((B0, mb), dtype=bool)
    planted[1, [2, 9]] = True                 # two outliers
    planted[3, :] = True                      # every row displaced
    data[planted] += 50.0
    if single:
        B0, data, planted = 1, data[1:2], planted[1:2]
    B = B0 * copies
    data = np.tile(data, (copies, 1))
    out = np.flatnonzero(np.tile(planted, (copies, 1)).reshape(-1))

    def f_(o, x):       # (a trial point of the block whose rows are all displaced may overflow exp: the loop refuses such a step)
        p = x.reshape(B, nb)
        with np.errstate(over="ignore", invalid="ignore"):
            o[:] = (p[:, 0:1] * np.exp(-p[:, 1:2] * t[None, :]) + p[:, 2:3] - data).reshape(-1)

    def g_(J, x):
        p = x.reshape(B, nb)
        with np.errstate(over="ignore", invalid="ignore"):
            e = np.exp(-p[:, 1:2] * t[None, :])
        v = J.data.reshape(B, nb, mb)
        v[:, 0, :] = e
        v[:, 1, :] = -p[:, 0:1] * t[None, :] * e
        v[:, 2, :] = 1.0

    x0 = np.tile(np.array([4.0, 1.0, 0.0]), B)
    name = "blocks" + (" single" if single else "") + ("" if copies == 1 else " x%d" % copies)
    return Case(name, "block", B * mb, B * nb, x0, f_, g_, lambda: lsq.BlockDiagonal(B, mb, nb), out, 122)


def global_case(displaced=True):
    """displaced=False: the same data without the three displaced rows (a plain weighted fit of them is dragged to a corner
    where the model is degenerate: fine for comparing bits, useless for comparing with a numpy inverse)."""
    B, mb, nb, ng = 4, 10, 2, 3
    m, n = B * mb, B * nb + ng
    rng = np.random.default_rng(131)
    t = np.linspace(0.2, 3.0, mb)
    amp, off = rng.uniform(3.0, 6.0, B), rng.uniform(-0.5, 0.5, B)
    k, s1, s2 = 1.1, 0.3, -0.05
    data = amp[:, None] * np.exp(-k * t)[None, :] + off[:, None] + (s1 * np.sin(3 * t) + s2 * np.cos(3 * t))[None, :] \
        + 0.03 * rng.standard_normal((B, mb))
    out = np.array([4, 2 * mb + 1, 2 * mb + 7]) if displaced else np.array([], dtype=np.int64)
    if displaced:
        data[0, 4] += 50.0
        data[2, [1, 7]] -= 50.0

    def f_(o, x):
        p, g = x[:B * nb].reshape(B, nb), x[B * nb:]
        o[:] = (p[:, 0:1] * np.exp(-g[0] * t)[None, :] + p[:, 1:2] + (g[1] * np.sin(3 * t) + g[2] * np.cos(3 * t))[None, :]
                - data).reshape(-1)

    def g_(J, x):
        p, g = x[:B * nb].reshape(B, nb), x[B * nb:]
        e = np.exp(-g[0] * t)
        v = J.data[:B * mb * nb].reshape(B, nb, mb)
        v[:, 0, :] = e[None, :]
        v[:, 1, :] = 1.0
        C = J.border
        C[:, 0] = (-p[:, 0:1] * (t * e)[None, :]).reshape(-1)
        C[:, 1] = np.tile(np.sin(3 * t), B)
        C[:, 2] = np.tile(np.cos(3 * t), B)

    x0 = np.concatenate([np.tile(np.array([4.0, 0.0]), B), [0.8, 0.0, 0.0]])
    return Case("global", "bordered", m, n, x0, f_, g_, lambda: lsq.BorderedBlockDiagonal(B, mb, nb, ng), out, 132)


CASES = {"decay": decay_case, "line": line_case, "blocks": blocks_case, "global": global_case}


def gradient_tolerance(case, loss, c, sigma):
    """g_tol of the runs that must end on the gradient: 1e-6 of its size at the start.  (An absolute 1e-8 is below what a
    trust-region loop can resolve here: a step's gain must exceed eps * ssr to be accepted, which stops the runs near
    |g| = sqrt(eps ssr |H|), 1e-5 .. 1e-4 for these costs of 1e2 .. 1e6.)"""
    return 1e-6 * robust_gradient(case, case.x0, loss, c, sigma)[1]


# The flag g_converged speaks about the iterate before the last step; nothing in the loop bounds the gradient AFTER it.  What
# does: the step solves (J~'J~ + D) dx = -g, so the new gradient is D dx plus the inner solver's residual plus the curvature
# term, each a fraction of |g| near a minimiser -- LSMR() stops its inner solve loosely and was seen at 1.8 |g|.  A factor of
# 10 is an order-of-magnitude guard against a last step that throws the fit away, not a certificate.
LAST_STEP_FACTOR = 10.0


def measured_point(r, x0):
    """Where the loop measured the gradient that ended it: the iterate BEFORE the last step (the reference evaluates
    maxabs(J'f) at the top of an iteration, then steps, then assesses convergence: levenberg_marquardt.jl:102-144)."""
    k = r.iterations
    return np.array(r.trace["x"][k - 2]) if k >= 2 else np.array(x0)


# ------------------------------------------------------------------------------------------------ the oracle's view of a case
def oracle_problem(O, case, f_, g_):
    """(Mat, f, g) for oracle.optimize: its g gets the flat value array, the host g_ the container around it."""
    J = case.new_J()
    if case.kind == "dense":
        mat = O.Mat(dense=J)

        def g(vals, x):
            g_(vals.reshape((case.m, case.n), order="F"), x)
    else:
        S = J if case.kind == "csc" else J.tocsc()
        mat = O.Mat(csc=(case.m, case.n, S.indptr, S.indices, np.zeros(S.nnz)))

        def g(vals, x):
            J.data = vals
            g_(J, x)
    return mat, f_, g
