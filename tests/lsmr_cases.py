"""The LSMR stop-rule cases shared by tests/test_lsmr_stops_host.py (certifies them without a device) and
tests/test_k_gpu_lsmr_stops.py (runs them on every iteration driver).  The seeds below were fixed on the CPU, from the twin
(tests/lsmr_reference.py) and the oracle alone, before any device run, and are never changed to suit one.

How a case reaches its stop BY CONSTRUCTION rather than by luck (a stop decided by round-off is not a test):

  threshold stops (rules 1 and 2, undamped)   A = J diag(P) is the operator the recurrence sees.  With its SVD A = U S V',
      y = sum_{i<k} c_i u_i  +  noise * sum_{i>=k} g_i u_i  +  resid * w,   w orthogonal to range(A),
      spans a Krylov space of dimension k up to `noise`: test1 (resid = 0) or test2 (resid = 1) sits at O(1e-2 .. 1) for
      k - 1 iterations and falls to O(noise) at iteration k -- far on either side of atol = btol = 1e-6 and of 2^-53.
      The choice of k sets the stopping iteration (odd, even, 1).
  threshold stops, damped   b = [y; 0] cannot be shaped that way, and btol = 0.5 against test1 <= 1 leaves no room for "misses
      by a factor 4 at an earlier iteration": a certified damped threshold stop is a stop at iteration 1.
  exact stops (0, 4, 5)   J = [diag(2^k); 0]: P is a power of two (damped: colsum + damp is a power of four on the column
      that y touches), every vector of the recurrence has one non-zero entry per block of rows and every sum one non-zero
      term, so beta, alpha, normr or normAr is 0.0 in ANY summation order.
  maxiter (7)   square, undamped, singular values graded over `cond`, generic y: the Krylov space has full dimension and
      nothing converges before iteration n = maxiter.  The operands are mild (6 x 6 with cond 5, 8 x 8 with cond 3): at
      iteration n the recurrence terminates, and on cond 1e3 the fp64 iterate there is 1e-6 .. 0.5 from the longdouble one.
  breakdown at iteration 2   two 3 x 2 / 3 x 3 operands with entries 0, +-1, +-2 on which every sum of the recurrence has
      ONE non-zero term and beta is 0.0 at the second iteration (found by the bounded search that
      tests/test_lsmr_stops_host.py describes; kept because the zero survives row permutations, rescalings and sums
      accumulated in longdouble).

`cases()` maps a name to a Case; `certify(name)` runs the twin in float64 and longdouble and the oracle and returns what the
device tests compare against; REUSE is the sequence of right-hand sides on ONE operand whose stops fall on iteration 0, 1, an
even one, an odd one and maxiter.
"""
import functools

import numpy as np

import lsmr_reference as R
from oracle import oracle as O

LD = np.longdouble


class Case:
    def __init__(self, name, J, y, damp, istop, note=""):
        self.name, self.istop, self.note = name, istop, note
        self.J = np.ascontiguousarray(J, dtype=np.float64)
        self.y = np.ascontiguousarray(y, dtype=np.float64)
        self.damp = None if damp is None else np.ascontiguousarray(damp, dtype=np.float64)
        self.m, self.n = self.J.shape

    @property
    def damped(self):
        return self.damp is not None

    @property
    def kind(self):
        return {0: "exact", 4: "exact", 5: "exact", 7: "maxiter"}.get(self.istop, "threshold")


def graded(m, n, cond, seed):
    """U diag(s) V' with s graded geometrically from 1 down to 1/cond, U and V Haar-distributed."""
    rng = np.random.default_rng(seed)
    k = min(m, n)
    U, _ = np.linalg.qr(rng.standard_normal((m, k)))
    V, _ = np.linalg.qr(rng.standard_normal((n, k)))
    return (U * np.logspace(0.0, -np.log10(cond), k)) @ V.T


def shaped_rhs(J, k, noise, resid, seed):
    """The right-hand side described in the module docstring for the undamped operator J diag(P)."""
    m, n = J.shape
    rng = np.random.default_rng(seed)
    cs = np.sum(J * J, axis=0)
    A = J * np.where(cs > 0, 1.0 / np.sqrt(np.where(cs > 0, cs, 1.0)), 0.0)
    U, s, _ = np.linalg.svd(A, full_matrices=True)
    r = int(np.sum(s > 1e-12 * s[0]))
    c = 1.0 + rng.random(k)
    y = U[:, :k] @ c
    if r > k:
        y = y + noise * (U[:, k:r] @ rng.standard_normal(r - k))
    if resid:
        assert m > r
        w = U[:, r:] @ rng.standard_normal(m - r)
        y = y + resid * w / np.linalg.norm(w) * np.linalg.norm(c)
    return y


def diag_pow2(m=16, n=12, empty=None):
    J = np.zeros((m, n))
    for k in range(n):
        J[k, k] = 2.0 ** (k - 4)
    if empty is not None:
        J[:, empty] = 0.0
    return J


def unit(m, *idx):
    e = np.zeros(m)
    for i in idx:
        e[i] = 1.0
    return e


def _build():
    C = {}

    def add(name, J, y, damp, istop, note=""):
        C[name] = Case(name, J, y, damp, istop, note)

    # ---- exact stops on [diag(2^k); 0], 16 x 12 ------------------------------------------------------------------------
    D = diag_pow2()
    n = D.shape[1]
    add("zero_y", D, np.zeros(16), None, 0, "b == 0")
    add("zero_y_damped", D, np.zeros(16), np.full(n, 0.5), 0, "b == 0")
    add("zero_Atb", D, unit(16, 13), None, 0, "A'b == 0, b != 0")
    add("zero_Atb_damped", D, unit(16, 13, 15), np.full(n, 1.0), 0, "A'b == 0, b != 0")
    add("exact4_e2", D, unit(16, 2), None, 4, "beta == 0 at iteration 1: normr == 0")
    dz = np.full(n, 1.0)
    dz[2] = 0.0
    add("exact4_e2_damped", D, unit(16, 2), dz, 4, "damp == 0 on the one column y touches: beta == 0, normr == 0")
    add("exact5_e2_e13", D, unit(16, 2, 13), None, 5, "alpha == 0 at iteration 1: normAr == 0, normr == 1")
    # colsum + damp = 4^-2 + 3 * 4^-2 = 4^-1 on column 2: P[2] = 2 exactly
    add("exact5_e2_damped", D, unit(16, 2), np.full(n, 3.0 * 4.0 ** -2), 5, "alpha == 0 at iteration 1: normAr == 0")
    De = diag_pow2(empty=3)
    add("exact5_emptycol", De, np.ones(16), None, 5, "P[3] == 0 for an empty column; alpha == 0 at iteration 1")
    dd = np.full(n, 3.0 * 4.0 ** -2)
    dd[3] = 0.0
    add("exact5_emptycol_damped", De, unit(16, 2), dd, 5, "P[3] == 0: colsum + damp == 0 on the empty column; alpha == 0")
    # ---- beta == 0 at iteration 2 (v and alpha left alone at a NON-first iteration) --------------------------------------
    add("exact5_beta0_it2", np.array([[0.0, 0.0], [-2.0, 1.0], [0.0, 1.0]]), np.array([0.0, 0.0, 2.0]), None, 5,
        "beta == 0 at iteration 2, normAr == 0")
    add("exact5_beta0_it2_3x3", np.array([[-1.0, -2.0, 0.0], [-2.0, 0.0, 0.0], [0.0, 0.0, -2.0]]), np.array([0.0, 1.0, 0.0]),
        None, 5, "beta == 0 at iteration 2, normAr == 0")

    # ---- threshold stops, undamped, at a chosen iteration --------------------------------------------------------------
    T = graded(60, 12, 2.0, 101)
    add("rule1_it1", T, shaped_rhs(T, 1, 1e-9, 0.0, 111), None, 1)
    add("rule1_it4", T, shaped_rhs(T, 4, 1e-9, 0.0, 112), None, 1)
    add("rule1_it5", T, shaped_rhs(T, 5, 1e-9, 0.0, 113), None, 1)
    add("rule2_it1", T, shaped_rhs(T, 1, 1e-9, 1.0, 114), None, 2)
    add("rule2_it2", T, shaped_rhs(T, 2, 1e-9, 1.0, 115), None, 2)
    add("rule2_it3", T, shaped_rhs(T, 3, 1e-9, 1.0, 116), None, 2)
    W = graded(9, 24, 4.0, 102)         # wide: rank 9, n = maxiter = 24
    add("rule1_wide_it3", W, shaped_rhs(W, 3, 1e-9, 0.0, 117), None, 1)
    # ---- threshold stops, damped: iteration 1 ----------------------------------------------------------------------------
    # rule 2: J'J + damp = 1.3 (I + O(1e-8)) off an empty column, y generic (test1 stays near 1): test2 = O(1e-8) after one step
    rng = np.random.default_rng(300)
    Q, _ = np.linalg.qr(rng.standard_normal((60, 12)))
    Jq = Q + 3e-9 * rng.standard_normal((60, 12))
    add("rule2_damped_it1", Jq, rng.standard_normal(60), np.full(12, 0.3), 2)
    Je = Jq.copy()
    Je[:, 3] = 0.0
    de = np.full(12, 0.3)
    de[3] = 0.0
    add("rule2_damped_emptycol_it1", Je, rng.standard_normal(60), de, 2, "P[3] == 0 in a threshold stop")
    # rule 1: singular values within 5 %, y consistent, damping 0.2 % of the column sums: test1 = O(0.05) after one step
    Jc = graded(60, 12, 1.05, 400)
    add("rule1_damped_it1", Jc, Jc @ np.random.default_rng(407).standard_normal(12), 0.002 * np.sum(Jc * Jc, axis=0), 1)
    # ---- maxiter: square, undamped, generic y; and the reuse sequence on the same 6 x 6 operand ------------------------
    S6 = graded(6, 6, 5.0, 202)
    add("rule7_s6", S6, np.random.default_rng(1202).standard_normal(6), None, 7)
    S8 = graded(8, 8, 3.0, 200)
    add("rule7_s8", S8, np.random.default_rng(1200).standard_normal(8), None, 7)
    add("s6_zero", S6, np.zeros(6), None, 0)
    add("s6_it1", S6, shaped_rhs(S6, 1, 1e-9, 0.0, 121), None, 1)
    add("s6_it2", S6, shaped_rhs(S6, 2, 1e-9, 0.0, 122), None, 1)
    add("s6_it3", S6, shaped_rhs(S6, 3, 1e-9, 0.0, 123), None, 1)
    return C


REUSE = ("s6_zero", "s6_it1", "s6_it2", "s6_it3", "rule7_s6", "s6_zero")     # iteration 0, 1, 2, 3, 6 = maxiter, 0 again


@functools.lru_cache(maxsize=None)
def cases():
    return _build()


def rel_err(x, x_hp):
    """The tier's metric ||x - x_hp|| / ||x_hp|| in longdouble (x_hp == 0: max |x|, which must then be 0)."""
    x, x_hp = np.asarray(x, dtype=LD), np.asarray(x_hp, dtype=LD)
    nh = np.sqrt(x_hp @ x_hp)
    d = x - x_hp
    return float(np.sqrt(d @ d) / nh) if nh > 0 else float(np.max(np.abs(x)))


def jacobi(J, damp=None):
    """The default preconditioner in fp64 from the oracle's column sums (what O.ldiv forms itself)."""
    s = O.colsumabs2(O.Mat(dense=J))
    if damp is not None and np.any(damp != 0):
        s = s + damp
    return np.where(s > 0, 1.0 / np.sqrt(np.where(s > 0, s, 1.0)), 0.0)


class Certified:
    pass


@functools.lru_cache(maxsize=None)
def certify(name):
    """Everything the tests compare against, computed once per case: the twins' records, the oracle's solve and stop code,
    x_hp at the certified iteration count, e_ref and the margins."""
    c = cases()[name]
    z = Certified()
    z.case = c
    z.f64 = R.ldiv_lsmr(c.J, c.y, c.damp)
    z.ld = R.ldiv_lsmr(c.J, c.y, c.damp, dtype=LD)
    A = O.Mat(dense=c.J)
    res = O.ldiv(O.LSMR, A, c.y, c.damp) if c.damped else O.ldiv(O.LSMR, A, c.y)
    z.x_oracle, z.nmul_oracle = res[1], res[2]
    z.damp_after_oracle = res[3] if c.damped else None
    raw = O.lsmr(A, c.y, diag=np.sqrt(c.damp) if c.damped else None, P=jacobi(c.J, c.damp),
                 btol=R.BTOL_DAMPED if c.damped else R.BTOL, maxiter=z.f64.maxiter)
    z.oracle_iter, z.oracle_istop = raw["iter"], raw["istop"]
    z.iter, z.istop, z.nmul = z.f64.iter, z.f64.istop, 2 * z.f64.iter
    z.x_hp = R.ldiv_lsmr(c.J, c.y, c.damp, dtype=LD, iters=z.iter).x
    z.e_ref = rel_err(z.x_oracle, z.x_hp)
    z.passed, z.missed = R.margins(z.f64)
    return z
