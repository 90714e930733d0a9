"""Shared by tests/test_dense_qr_covariance_host.py and tests/test_n_gpu_dense_qr_covariance.py: the operands, the longdouble
reference and the fp64 e_ref of the covariance from the QR() factor (lsq_dense_qr_covariance).  Metrics and rule are those of
tests/accuracy_common.py, unchanged: ac.judge(ac.cov_pieces(.., k = n)), e_dev <= 16 max(e_ref, min(max(16, n), 64) 2^-53).

    H        inv(R) inv(R)' from a numpy.longdouble Householder R (the loop of hp.lstsq_qr) -- NOT hp.inv_gram, whose
             longdouble Cholesky of J'J has no digits left at 9 decades
    e_ref    fp64: numpy.linalg.qr(A, mode="r"), a triangular solve against I, X X'
    families ac.FAMILIES, ill6 / ill9 (ac.ill_matrix with 6 / 9 decades), and shuffled-graded: the graded operand with its
             columns permuted by a seeded permutation -- without it every pivoted factorisation of these operands has
             jp = identity (graded columns are already in pivot order), and a permutation mistake hides
"""
import functools

import numpy as np
import scipy.linalg

import accuracy_common as ac
import hp_reference as hp

# n = 1 and the one-workgroup path; one tile on the one-stage path; two-stage without a CholeskyQR2 panel; one CholeskyQR2 panel,
# a ragged second tile and one k_tri_level level; three tiles and two levels; four tiles; TSQR
SHAPES = [(40, 1), (50, 3), (90, 31), (300, 65), (500, 130), (700, 200), (33000, 8)]
FAMILIES = ac.FAMILIES + ("ill6", "ill9", "shuffled-graded")
ILL_FAMILIES = ("ill", "ill6", "ill9")
CASES = [(m, n, fam) for (m, n) in SHAPES for fam in FAMILIES if not (n == 1 and "graded" in fam)]   # (ac.grading: k - 1 = 0)


def shuffle_perm(m, n):
    return np.random.default_rng(ac.dense_seed(m, n) + 1).permutation(n)


def operand(family, m, n):
    """(A, f): the fp64 operand (column-major) and a standard normal residual (scaled with the operand in far+ / far-)."""
    seed = ac.dense_seed(m, n)
    if family in ac.FAMILIES:
        op = ac.dense_operand(family, m, n, seed)
        return op.J, op.y
    if family == "shuffled-graded":
        op = ac.dense_operand("graded", m, n, seed)
        return np.asfortranarray(op.J[:, shuffle_perm(m, n)]), op.y
    rng = np.random.default_rng(seed)
    A = ac.ill_matrix(rng, m, n, decades={"ill6": 6.0, "ill9": 9.0}[family])
    return np.asfortranarray(A), rng.standard_normal(m)


def householder_r(A):
    """The n x n triangle of a longdouble Householder QR of A (fp64, converted exactly, or longdouble): hp.lstsq_qr's loop."""
    A = hp.ld(A)
    n = A.shape[1]
    RT = np.ascontiguousarray(A.T)
    for j in range(n):
        v = RT[j, j:].copy()
        alpha = np.sqrt(v @ v)
        if alpha == 0:
            raise np.linalg.LinAlgError("longdouble QR: column %d is zero" % j)
        v[0] += alpha if v[0] >= 0 else -alpha
        v = v / np.sqrt(v @ v)
        RT[j:, j:] -= 2 * np.outer(RT[j:, j:] @ v, v)
    return np.triu(RT.T[:n, :n])


def inv_gram_qr(A):
    """inv(A'A) in longdouble without forming A'A."""
    R = householder_r(A)
    Xi = hp.solve_upper(R, np.eye(R.shape[0], dtype=hp.LD))
    return Xi @ Xi.T


def fp64_qr_route(A):
    """e_ref's route, all fp64: LAPACK's unpivoted Householder R, one triangular solve against I, X X'."""
    R = np.linalg.qr(A, mode="r")
    X = scipy.linalg.solve_triangular(R, np.eye(R.shape[0]), lower=False)
    return X @ X.T


def tri_inv_blocked(R):
    """inv(R) of an upper triangle by the block recursion of the device (X12 = -X11 (R12 X22)), fp64."""
    n = R.shape[0]
    if n == 1:
        return np.array([[1.0 / R[0, 0]]])
    h = n // 2
    X11, X22 = tri_inv_blocked(R[:h, :h]), tri_inv_blocked(R[h:, h:])
    X = np.zeros((n, n))
    X[:h, :h], X[h:, h:] = X11, X22
    X[:h, h:] = -X11 @ (R[:h, h:] @ X22)
    return X


def fp64_pivoted_route(A):
    """A second fp64 route, the device's algebra: pivoted LAPACK QR, block-recursive inverse, X X', un-permute."""
    R, P = scipy.linalg.qr(A, mode="r", pivoting=True)
    n = A.shape[1]
    X = tri_inv_blocked(np.triu(R[:n, :n]))
    C = np.empty((n, n))
    C[np.ix_(P, P)] = X @ X.T
    return C


class Ref:
    """One operand with its longdouble inv(A'A), the fp64 e_ref route and both variances.  A_eff: the operand the handle
    means, in longdouble, where that is not fl(A) (a column-scaled handle)."""

    def __init__(self, A, f, A_eff=None):
        m, n = A.shape
        self.A, self.f, self.m, self.n = A, f, m, n
        self.H = inv_gram_qr(A if A_eff is None else A_eff)
        self.R = fp64_qr_route(A)
        self.s2_hp = ac.s2_of(f, m - n) if m > n else None
        self.s2 = float(f @ f) / (m - n) if m > n else None

    def scales(self, with_f):
        return (self.s2_hp, self.s2) if with_f else (hp.LD(1), 1.0)

    def pieces(self, name, cov, se, with_f):
        """cov, se: fp64 arrays (n x n, n) that already carry the variance when with_f."""
        s_hp, s64 = self.scales(with_f)
        return ac.cov_pieces(name, cov, se, s64 * self.R, self.H * s_hp, self.n)


@functools.lru_cache(maxsize=None)
def ref(family, m, n):
    return Ref(*operand(family, m, n))
