"""Shared by tests/test_borderedqr_covariance_host.py (no device) and tests/test_w_gpu_borderedqr_covariance.py: the cases, the
longdouble reference, the fp64 e_ref and the numpy fp64 twin of lsq_bordered_qr_covariance (lsq_cov_bordered.hip).

The rule is the accuracy tier's, unchanged: ac.judge, e_dev <= 16 max(e_ref, min(max(16, k), 64) 2^-53), in the metric of
ac.cov_err / ac.stderr_err, per piece:
    each Cov_bb with its standard errors     k = nb
    the shared block with its standard errors k = ng
    each cross block Cov_bg                   k = nb + ng, metric max |X_ij - H_ij| / sqrt(H_ii H_jj), i over the block's
                                              locals, j over the shared columns
    H      qr_cov_common.inv_gram_qr of the stacked dense matrix (longdouble Householder), times the longdouble s^2
    e_ref  qr_cov_common.fp64_qr_route of the same matrix (LAPACK's Householder R, a triangular solve, X X')
Neither comes from the code under test.

Shapes (B, mb, nb, ng) have B (mb - nb) >= ng -- else F has fewer rows than columns --, the `ill` families also
mb >= nb + ng (ac.ill_matrix).  Families: plain and graded (ac.bb_operand) on BRANCH_SHAPES, ill (three decades) on ILL_SHAPES,
ill6 (borderedqr_common.ill6_operands, six decades: cond(J'J) = 1e12) on borderedqr_common.ILL6_SHAPES.

The twin follows the device steps in fp64: borderedqr_common.eliminate_block with zero damping per block, numpy.linalg.qr of
the F stack, Cgg = inv(R_g) inv(R_g)', T_b = inv(R_b) W_b, P_b = T_b Cgg, Cov_bb = inv(R_b) inv(R_b)' + P_b T_b',
Cov_bg = -P_b, everything times s^2."""
import functools

import numpy as np
import scipy.linalg

import accuracy_common as ac
import borderedqr_common as bqc
import hp_reference as hp
import qr_cov_common as qc
import schur_common as sc

# one column each, 32-row chunks | m - n = 1 | wavefront path, 64-row chunks | last nb on the wavefront path, ragged second chunk
# | exactly one border tile | workgroup path, a second tile of one column | three tiles | nb = 64 | a grid that ends inside a
# workgroup of four | B = 1
BRANCH_SHAPES = [(1, 3, 1, 1), (2, 2, 1, 1), (3, 40, 5, 31), (3, 33, 16, 32), (2, 70, 16, 64), (3, 100, 17, 65), (4, 100, 33, 129),
                 (5, 110, 64, 200), (65, 12, 5, 64), (1, 130, 64, 63)]
ILL_SHAPES = [(1, 3, 1, 1), (3, 40, 5, 31), (3, 100, 17, 65), (5, 96, 5, 3), (3, 96, 64, 32)]
CASES = ([(fam, s) for s in BRANCH_SHAPES for fam in ("plain", "graded")] + [("ill", s) for s in ILL_SHAPES] +
         [("ill6", s) for s in bqc.ILL6_SHAPES])
for _f, (_B, _mb, _nb, _ng) in CASES:
    assert _B * (_mb - _nb) >= _ng and (not _f.startswith("ill") or _mb >= _nb + _ng)


def case_id(case):
    return "%s-%s" % (case[0], "x".join(str(v) for v in case[1]))


@functools.lru_cache(maxsize=None)
def operand(family, shape):
    """An ac.Operand: J (a BorderedBlockDiagonal), y (the residual of the with-f cases), and for graded V, s."""
    B, mb, nb, ng = shape
    if family == "ill6":
        return bqc.ill6_operands(B, mb, nb, ng)["random"]
    return ac.bb_operand(family, B, mb, nb, ng, sc.acc_seed(B, nb, ng))


class Parts:
    """A covariance in pieces: blocks (B arrays nb x nb), shared (ng x ng), stderr (n), cross ((B nb) x ng); any may be None."""

    def __init__(self, blocks=None, shared=None, stderr=None, cross=None):
        self.blocks, self.shared, self.stderr, self.cross = blocks, shared, stderr, cross

    @classmethod
    def of_full(cls, C, B, nb, ng):
        """The pieces of a full n x n matrix in parameter order."""
        L = B * nb
        return cls([C[b * nb:(b + 1) * nb, b * nb:(b + 1) * nb] for b in range(B)], C[L:, L:], np.sqrt(np.diag(C)), C[:L, L:])

    @classmethod
    def of_dev(cls, cv):
        """... of a lsq.BorderedCovariance or lsq.Covariance."""
        blocks = None if cv.cov is None else [cv.block(b) for b in range(cv.nblocks)]
        return cls(blocks, None if cv.cov is None else cv.shared, cv.stderr, getattr(cv, "cross", None))

    def scaled(self, s2):
        mul = lambda a, f: None if a is None else a * f
        return Parts(None if self.blocks is None else [b * s2 for b in self.blocks], mul(self.shared, s2),
                     mul(self.stderr, np.sqrt(s2)), mul(self.cross, s2))


def cross_err(X, H, rows, cols):
    """max |X_ij - H_ij| / sqrt(H_ii H_jj), i in rows, j in cols; X: the panel alone, H: the full longdouble matrix."""
    sd = np.sqrt(np.diag(H))
    return float(np.max(np.abs(hp.ld(X) - H[rows, cols]) / np.outer(sd[rows], sd[cols])))


class Ref:
    """One operand with its longdouble inv(J'J), the fp64 e_ref route and both variances.  scaled: the handle means
    V diag(s) unrounded; the fp64 comparator still works on J = fl(V diag(s))."""

    def __init__(self, op, scaled=False):
        J = op.J
        self.B, self.mb, self.nb, self.ng = J.nblocks, J.mb, J.nb, J.ng
        self.m, self.n = J.shape
        A = J.toarray()
        self.A = A
        self.H = qc.inv_gram_qr((hp.ld(op.V.toarray()) * hp.ld(op.s)) if scaled else A)
        self.R = qc.fp64_qr_route(A)
        self.f = op.y
        self.s2_hp = ac.s2_of(op.y, self.m - self.n)
        self.s2 = float(op.y @ op.y) / (self.m - self.n)

    def scales(self, with_f):
        return (self.s2_hp, self.s2) if with_f else (hp.LD(1), 1.0)

    def pieces(self, parts, with_f, e_ref_of=None):
        """(name, e_dev, e_ref, k) for whatever `parts` holds; it already carries the variance when with_f.  e_ref_of: another
        fp64 full matrix (unit variance) in the place of the Householder route's."""
        B, nb, ng = self.B, self.nb, self.ng
        s_hp, s64 = self.scales(with_f)
        H, R = self.H * s_hp, s64 * (self.R if e_ref_of is None else e_ref_of)
        L, sh = B * nb, slice(B * nb, B * nb + ng)
        out = []
        for b in range(B):
            sl = slice(b * nb, (b + 1) * nb)
            if parts.blocks is not None:
                out.append(("block %d" % b, ac.cov_err(parts.blocks[b], H[sl, sl]), ac.cov_err(R[sl, sl], H[sl, sl]), nb))
            if parts.stderr is not None:
                out.append(("block %d stderr" % b, ac.stderr_err(parts.stderr[sl], H[sl, sl]),
                            ac.stderr_err(np.sqrt(np.diag(R[sl, sl])), H[sl, sl]), nb))
            if parts.cross is not None:
                out.append(("cross %d" % b, cross_err(parts.cross[sl], H, sl, sh), cross_err(R[sl, sh], H, sl, sh), nb + ng))
        if parts.shared is not None:
            out.append(("shared", ac.cov_err(parts.shared, H[sh, sh]), ac.cov_err(R[sh, sh], H[sh, sh]), ng))
        if parts.stderr is not None:
            out.append(("shared stderr", ac.stderr_err(parts.stderr[L:], H[sh, sh]),
                        ac.stderr_err(np.sqrt(np.diag(R[sh, sh])), H[sh, sh]), ng))
        return out

    def distances(self, pa, pb, with_f):
        """(name, distance) between two results in the metric of their pieces: by the triangle inequality at most
        e(pa) + e(pb).  Only what both hold."""
        B, nb, ng = self.B, self.nb, self.ng
        H = self.H * self.scales(with_f)[0]
        sd = np.sqrt(np.diag(H))
        L, sh = B * nb, slice(B * nb, B * nb + ng)
        rel = lambda D, r, c: float(np.max(np.abs(D) / np.outer(sd[r], sd[c])))
        out = []
        for b in range(B):
            sl = slice(b * nb, (b + 1) * nb)
            if pa.blocks is not None and pb.blocks is not None:
                out.append(("block %d" % b, rel(hp.ld(pa.blocks[b]) - hp.ld(pb.blocks[b]), sl, sl)))
            if pa.cross is not None and pb.cross is not None:
                out.append(("cross %d" % b, rel(hp.ld(pa.cross[sl]) - hp.ld(pb.cross[sl]), sl, sh)))
        if pa.shared is not None and pb.shared is not None:
            out.append(("shared", rel(hp.ld(pa.shared) - hp.ld(pb.shared), sh, sh)))
        if pa.stderr is not None and pb.stderr is not None:
            d = np.abs(hp.ld(pa.stderr) - hp.ld(pb.stderr)) / sd
            out += [("block %d stderr" % b, float(np.max(d[b * nb:(b + 1) * nb]))) for b in range(B)]
            out.append(("shared stderr", float(np.max(d[L:]))))
        return out


@functools.lru_cache(maxsize=None)
def ref(family, shape, scaled=False):
    return Ref(operand(family, shape), scaled)


def beyond(pieces):
    """The largest e / bound over the pieces: > 1 means outside the rule."""
    return bqc.beyond(pieces)


# ------------------------------------------------------------------------------------------ the twin
def twin(J, colscale=None, plant=None):
    """(Parts with unit variance, 0, rank), or (None, the 1-based stacked column of a failing local, None).  colscale: the
    handle holds V = J and means V diag(colscale).  plant: None, or a mistake the rule must catch: "cross-sign" (Cov_bg = +P_b)
    or "no-border-term" (Cov_bb without P_b T_b')."""
    B, mb, nb, ng = J.nblocks, J.mb, J.nb, J.ng
    s = np.ones(B * nb + ng) if colscale is None else np.asarray(colscale, dtype=np.float64)
    sg = s[B * nb:]
    parts, fail = [], 0
    with np.errstate(all="ignore"):
        for b in range(B):
            sl = slice(b * nb, (b + 1) * nb)
            R, W, _, F, _, bad = bqc.eliminate_block(J.block(b) * s[sl], J.border_block(b) * sg, np.zeros(mb), np.zeros(nb))
            if bad and not fail:
                fail = b * nb + bad
            parts.append((R, W, F))
    if fail:
        return None, fail, None
    Rg = np.linalg.qr(np.vstack([p[2] for p in parts]), mode="r")
    rank = int(np.sum(np.abs(np.diag(Rg)) > ng * np.finfo(np.float64).eps * np.max(np.abs(np.diag(Rg)))))
    Xg = scipy.linalg.solve_triangular(Rg, np.eye(ng), lower=False)
    Cgg = Xg @ Xg.T
    blocks, cross = [], np.empty((B * nb, ng))
    for b, (R, W, _) in enumerate(parts):
        X = scipy.linalg.solve_triangular(R, np.eye(nb), lower=False)
        T = scipy.linalg.solve_triangular(R, W, lower=False)
        P = T @ Cgg
        blocks.append(X @ X.T + (0.0 if plant == "no-border-term" else P @ T.T))
        cross[b * nb:(b + 1) * nb] = P if plant == "cross-sign" else -P
    se = np.sqrt(np.concatenate([np.diag(C) for C in blocks] + [np.diag(Cgg)]))
    return Parts(blocks, Cgg, se, cross), 0, rank


def normal_equations_route(A):
    """inv(A'A) the way the Cholesky-based entries form it, all fp64: Cholesky of A'A, the inverse of the factor, X X'.
    None where the factorisation breaks down."""
    try:
        U = np.linalg.cholesky(A.T @ A).T
    except np.linalg.LinAlgError:
        return None
    X = scipy.linalg.solve_triangular(U, np.eye(U.shape[0]), lower=False)
    return X @ X.T


def duplicated_border_case():
    """A plain (3, 40, 5, 31) operand whose last border column repeats the one before: the locals are fine, the transformed
    border has rank ng - 1."""
    B, mb, nb, ng = 3, 40, 5, 31
    J = sc.make_bb(B, mb, nb, ng, 5)
    J.border[:, ng - 1] = J.border[:, ng - 2]
    return J
