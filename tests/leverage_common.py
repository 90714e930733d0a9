"""Shared by tests/test_leverage_host.py and tests/test_y_gpu_leverage.py: the longdouble reference, the fp64 e_ref and the
numpy twins of the leverage entry points (lsq_dense_qr_leverage, lsq_solver_leverage; lsq_leverage.hip).  The operands are
those of tests/qr_cov_common.py (dense) and tests/accuracy_common.py (block-diagonal); the rule is the accuracy tier's,
unchanged: ac.judge with k = n (nb per block),  e_dev <= 16 max(e_ref, min(max(16, k), 64) 2^-53).

    metric   e(q) = max_i |q_i - q_hp,i| / q_hp,i, in longdouble (se: the same on sqrt(s2 q))
    q_hp     longdouble: qc.householder_r, hp.solve_upper against I for X = inv(R), row sums of squares of A X
    e_ref    fp64: numpy.linalg.qr(J, mode="r"), scipy.linalg.solve_triangular(R, A.T, trans="T"), column sums of squares
    twins    the device's algebra in numpy fp64 -- dense: pivoted LAPACK QR, qc.tri_inv_blocked, A[:, P] @ X, row sums of squares;
             block: ac.standin_factor on ac.standin_gram, the explicit inverse, A X, and the same once more on A X
             (CholeskyQR2, as k_bd_lev).  They certify on the CPU that the bound is
             within reach of a correct fp64 implementation on every case, and with a planted mistake that it is not vacuous.
    diag     the numpy twin of k_lev_diag in the operation order include/lsqhip.h fixes: bit for bit
"""
import functools

import numpy as np
import scipy.linalg

import accuracy_common as ac
import hp_reference as hp
import qr_cov_common as qc

CASES = qc.CASES
MISTAKES = ("no-permutation", "inverse-permutation", "junk-below-diagonal", "strict-k", "no-colscale")
TILE = 64


def lev_err(q, q_hp):
    q, q_hp = hp.ld(q), hp.ld(q_hp)
    return float(np.max(np.abs(q - q_hp) / q_hp))


def q_hp(J_eff, A=None):
    """a' inv(J'J) a for the rows a of A (None: of J) in longdouble, without forming J'J."""
    R = qc.householder_r(J_eff)
    X = hp.solve_upper(R, np.eye(R.shape[0], dtype=hp.LD))
    Z = hp.ld(J_eff if A is None else A) @ X
    return np.sum(Z * Z, axis=1)


def q_fp64(J, A=None):
    """e_ref's route, all fp64."""
    R = np.linalg.qr(J, mode="r")
    W = scipy.linalg.solve_triangular(R, (J if A is None else A).T, trans="T", lower=False)
    return np.sum(W * W, axis=0)


def q_normal_equations(J, A=None):
    """The route the entry point avoids: inv(J'J) formed in fp64."""
    A = J if A is None else A
    C = np.linalg.inv(J.T @ J)
    return np.einsum("ij,jk,ik->i", A, C, A)


def twin_dense(J, A=None, mistake=None, scale=None):
    """The device's algebra in fp64.  J: the operand the factor sees (a column-scaled handle: V * s); A: the rows (None: J's --
    then, with `scale`, they are staged as V[:, c] * s[c] like k_lev_tall does, V = J / s being passed as `A`).
    mistake: one of MISTAKES, planted."""
    m, n = J.shape
    R, P = scipy.linalg.qr(J, mode="r", pivoting=True)
    X = qc.tri_inv_blocked(np.triu(R[:n, :n]))
    rows = J if A is None else A
    if scale is not None and mistake != "no-colscale":
        rows = rows * scale
    if mistake == "no-permutation":
        staged = rows
    elif mistake == "inverse-permutation":
        staged = rows[:, np.argsort(P)]
    else:
        staged = rows[:, P]
    if mistake == "junk-below-diagonal":
        X = X + np.tril(np.full((n, n), 0.5 * np.max(np.abs(X))), -1)
    if mistake == "strict-k":                       # K < Jt instead of K <= Jt: the diagonal tiles of X never contribute
        X = X.copy()
        for t in range(0, n, TILE):
            X[t:t + TILE, t:t + TILE] = 0.0
    Z = staged @ X
    return np.sum(Z * Z, axis=1)


def _inv_upper(U):
    """inv(U) by back substitution, a reciprocal per pivot (ac.standin_inv's loop)."""
    n = U.shape[0]
    X = np.zeros((n, n))
    dinv = 1.0 / np.diag(U)
    for r in range(n - 1, -1, -1):
        e = np.zeros(n)
        e[r] = 1.0
        X[r] = (e - U[r, r + 1:] @ X[r + 1:]) * dinv[r]
    return X


def twin_block(Ab, second_pass=True):
    """One block of lsq_solver_leverage in fp64, CholeskyQR2: the streamed Gram, G = U'U with reciprocal square roots,
    X = inv(U), Z = A X; then the same on Z (G2 = Z'Z = U2'U2, X2 = inv(U2)) and the row sums of squares of Z X2.
    second_pass=False: the row sums of squares of Z -- one Cholesky of J_b'J_b, which squares the condition number."""
    Z = Ab @ _inv_upper(ac.standin_factor(ac.standin_gram(Ab)))
    if second_pass:
        Z = Z @ _inv_upper(ac.standin_factor(ac.standin_gram(Z)))
    return np.sum(Z * Z, axis=1)


def diag_twin(q, f, s2, n):
    """k_lev_diag: (se, t, cook) from (q, f, s2) in the header's operation order, every line one IEEE operation.  s2: a scalar
    or one value per row."""
    q, f = np.asarray(q, dtype=np.float64), np.asarray(f, dtype=np.float64)
    with np.errstate(all="ignore"):
        sd = np.sqrt(np.asarray(s2, dtype=np.float64))
        se = sd * np.sqrt(q)
        d = 1.0 - q
        t = f / (sd * np.sqrt(d))
        cook = ((t * t) * q) / (np.float64(n) * d)
    return se, t, cook


def diag_hp(q, f, s2, n):
    """The same in longdouble."""
    q, f, s2 = hp.ld(q), hp.ld(f), hp.ld(s2)
    sd = np.sqrt(s2)
    d = 1 - q
    t = f / (sd * np.sqrt(d))
    return sd * np.sqrt(q), t, t * t * q / (hp.LD(n) * d)


def pieces(name, q_dev, r, with_f=False, se_dev=None):
    """(name, e_dev, e_ref, k) of q against r.q_hp / r.q_ref and, with_f, of se against sqrt(s2 q)."""
    out = [(name, lev_err(q_dev, r.q_hp), lev_err(r.q_ref, r.q_hp), r.n)]
    if with_f:
        se_hp = np.sqrt(r.s2_hp * r.q_hp)
        se_ref = np.sqrt(r.s2 * r.q_ref)
        out.append((name + " se", lev_err(se_dev, se_hp), lev_err(se_ref, se_hp), r.n))
    return out


class Ref:
    """One operand (J fp64 as the handle holds it, f) with the longdouble and fp64 quadratic forms of the rows A (None: J's
    own).  J_eff: what the handle means in longdouble where that is not fl(J) (a column-scaled handle)."""

    def __init__(self, J, f, A=None, J_eff=None, A_eff=None):
        self.J, self.f, self.A = J, f, A
        self.m, self.n = J.shape
        self.q_hp = q_hp(J if J_eff is None else J_eff, A if A_eff is None else A_eff)
        self.q_ref = q_fp64(J, A)
        self.s2_hp = ac.s2_of(f, self.m - self.n) if self.m > self.n else None
        self.s2 = float(f @ f) / (self.m - self.n) if self.m > self.n else None


@functools.lru_cache(maxsize=None)
def ref(family, m, n):
    return Ref(*qc.operand(family, m, n))


def block_ref(op, b, scaled_handle=False):
    """Block b of an ac.bd_operand as a Ref (k = nb)."""
    J = op.J
    mb = J.mb
    Ab = np.asfortranarray(J.block(b))
    eff = ac.bd_effective(op, b, scaled_handle) if scaled_handle else None
    return Ref(Ab, op.y[b * mb:(b + 1) * mb], J_eff=eff)
