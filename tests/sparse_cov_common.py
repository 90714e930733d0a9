"""Operands and references shared by tests/test_sparse_covariance_host.py (no device) and tests/test_q_gpu_sparse_covariance.py
(lsq_sparse_gram / lsq_sparse_covariance, lsq_cov_sparse.hip).  Rule, metrics and families are the accuracy tier's
(tests/accuracy_common.py, tests/hp_reference.py), unchanged.

Operands are sparse with FULL COLUMN RANK BY CONSTRUCTION: a diagonal block (n rows, entries in [1, 2), so every column has a
row of its own) stacked on a random part of m - n rows -- ac.ragged_pattern (one full row, an empty column, an empty row) where
it fits (n >= 2, m - n >= 6), a dense random block otherwise (n = 1), or a band.
    plain    diagonal in [1, 2), random part N(0, 1)
    graded   plain, column j times 10^(-8 j / (n - 1)); also as a column-scaled handle: V plain, s the grading
    far+/-   plain times 2^100 / 2^-100 (f too: the same covariance up to the exact factor)
    ill      a band (diagonal block over four sub-diagonals of the random part), columns graded over 3 decades
"""
import functools

import numpy as np
import scipy.sparse as sp

import accuracy_common as ac
import hp_reference as hp

FAMILIES = ("plain", "graded", "far+", "far-", "ill")
SHAPES = [(40, 1), (50, 3), (90, 31), (200, 64), (300, 65), (500, 130), (1000, 321)]
CASES = [(m, n, fam) for (m, n) in SHAPES for fam in FAMILIES if not (fam in ("graded", "ill") and n == 1)]   # (ac.grading: n - 1 = 0)

# lsq_cov_sparse.hip: W = min(4, floor(160 KiB / 8 n)) wavefronts per workgroup, and the limit
GRAM_LDS_BUDGET, GRAM_MAX_N = 160 * 1024, 16384


def gram_waves(n):
    return max(1, min(4, GRAM_LDS_BUDGET // (8 * n)))


W_SWITCHES = [(5120, 5121), (6826, 6827), (10240, 10241)]       # (last n with W waves, first n with W - 1): 4|3, 3|2, 2|1


def seed_of(m, n):
    return 7000 + m + n


def pattern(m, n, seed, band=False):
    """The sparse operand of the plain family (scipy CSC, sorted, no stored zeros)."""
    rng = np.random.default_rng(seed)
    top = sp.diags(1.0 + rng.random(n), 0, shape=(n, n), format="csc")
    k = m - n
    if band:
        offs = [0, 1, 2, 5]
        low = sp.diags([rng.standard_normal(n) for _ in offs], [-o for o in offs], shape=(k, n), format="csc") if k >= 1 else None
    elif n >= 2 and k >= 6:
        low = ac.ragged_pattern(k, n, min(1.0, max(0.05, 6.0 / n)), seed + 1)
    else:
        low = sp.csc_matrix(rng.standard_normal((k, n)))
    S = sp.vstack([top, low]).tocsc() if low is not None else top
    S.sort_indices()
    S.eliminate_zeros()
    return S


class SparseOperand:
    """S: the effective Jacobian as stored (fp64, scipy CSC); f: the residual of the case; V, s: the same operand as a
    column-scaled handle (graded only: S = fl(V diag(s)), the handle itself means V diag(s))."""

    def __init__(self, S, f, V=None, s=None):
        self.S, self.f, self.V, self.s = S, f, V, s


def operand(family, m, n, seed):
    assert family in FAMILIES
    rng = np.random.default_rng(seed + 17)
    P = pattern(m, n, seed, band=(family == "ill"))
    f = rng.standard_normal(m)
    if family == "plain":
        return SparseOperand(P, f)
    if family in ("far+", "far-"):
        sc = 2.0 ** (100 if family == "far+" else -100)
        return SparseOperand((P * sc).tocsc(), f * sc)
    s = ac.grading(n, 8.0 if family == "graded" else 3.0)
    S = (P @ sp.diags(s)).tocsc()
    S.sort_indices()
    return SparseOperand(S, f, P, s) if family == "graded" else SparseOperand(S, f)


class Ref:
    """H = inv(A'A) in longdouble, R the same by numpy in fp64 (e_ref), and the variances of the case's residual."""

    def __init__(self, A, f, A_hp=None):
        m, n = A.shape
        self.A, self.f, self.m, self.n = A, f, m, n
        self.H = hp.inv_gram(A if A_hp is None else A_hp)
        self.R = np.linalg.inv(A.T @ A)
        self.s2_hp = ac.s2_of(f, m - n) if m > n else None
        self.s2 = float(f @ f) / (m - n) if m > n else None

    def pieces(self, name, cov, se, with_f):
        s_hp, s64 = (self.s2_hp, self.s2) if with_f else (hp.LD(1), 1.0)
        return ac.cov_pieces(name, cov, se, s64 * self.R, self.H * s_hp, self.n)


@functools.lru_cache(maxsize=8)
def case(family, m, n):
    op = operand(family, m, n, seed_of(m, n))
    return op, Ref(op.S.toarray(), op.f)


# ------------------------------------------------------------------------------------------ the Gram matrix, per entry
def gram_reference(S, colscale=None, damp=None):
    """(G, mag, K) of the upper triangle of J'J (+ diag damp), J = S diag(colscale): the value and the sum of absolute terms in
    longdouble, and K_kj = the number of rows columns k and j share.  Dense n x n arrays (lower triangle: zeros)."""
    A = hp.ld(S.toarray())
    if colscale is not None:
        A = A * hp.ld(colscale)
    G = np.triu(A.T @ A)
    mag = np.triu(np.abs(A).T @ np.abs(A))
    P = (S != 0).astype(np.int64)
    K = np.triu((P.T @ P).toarray())
    if damp is not None:
        G = G + np.diag(hp.ld(damp))
        mag = mag + np.diag(np.abs(hp.ld(damp)))
    return G, mag, K


def gram_twin(S, colscale=None, damp=None):
    """What k_sp_gram computes, in plain Python fp64: for column j the stored entries (i, v) in CSC order, for each the row i
    up to column j, acc[c] += v * w (a product, then an add: the library is built without contraction); then the scaling of
    the fused column-scaled handle, (acc_k s_k) s_j, and the damping on the diagonal."""
    S = S.tocsc()
    S.sort_indices()
    R = S.tocsr()
    R.sort_indices()
    m, n = S.shape
    G = np.zeros((n, n))
    for j in range(n):
        acc = np.zeros(n)
        for e in range(S.indptr[j], S.indptr[j + 1]):
            i, v = S.indices[e], S.data[e]
            for q in range(R.indptr[i], R.indptr[i + 1]):
                c = R.indices[q]
                if c > j:
                    break
                acc[c] = acc[c] + v * R.data[q]
        col = acc[:j + 1]
        if colscale is not None:
            col = (col * colscale[:j + 1]) * colscale[j]
        G[:j + 1, j] = col
        if damp is not None:
            G[j, j] = G[j, j] + damp[j]
    return G


def gram_excess(G, ref, mag, K, c):
    """max over the stored entries (k <= j) of |G - ref| / product_bound(K, c, mag); inf if an entry with K = 0 is not an exact
    zero (with damping: not exactly the damping)."""
    iu = np.triu_indices(G.shape[0])
    q, i = ac.product_excess(G[iu], ref[iu], K[iu], c, mag[iu])
    return q, (int(iu[0][i]), int(iu[1][i]))


def band_int(m, n, seed):
    """At most three entries per row, small integers: every sum of J'J is exact in fp64."""
    rng = np.random.default_rng(seed)
    diags = [rng.integers(1, 8, n).astype(float), rng.integers(-7, 8, n).astype(float), rng.integers(-7, 8, n).astype(float)]
    S = sp.diags(diags, [0, -1, -2], shape=(m, n), format="csc")
    S.sort_indices()
    S.eliminate_zeros()
    return S


def block_pattern(B, mb, nb, seed):
    """A block-diagonal pattern as a PLAIN CSC matrix: B dense mb x nb blocks."""
    rng = np.random.default_rng(seed)
    blocks = [rng.standard_normal((mb, nb)) + np.vstack([2.0 * np.eye(nb), np.zeros((mb - nb, nb))]) for _ in range(B)]
    S = sp.block_diag(blocks, format="csc")
    S.sort_indices()
    return S, blocks
