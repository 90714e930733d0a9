"""The accuracy tier's operands, metrics and acceptance rule, shared by tests/test_accuracy_host.py (no device) and
tests/test_h_gpu_accuracy.py.  The reference is tests/hp_reference.py (numpy.longdouble).

Metrics -- all in longdouble, per PIECE (each block; the shared part of a bordered handle separately), so that a small piece
cannot hide inside a large one:
    solve        e(x) = ||S (x - x_hp)||_2 / ||S x_hp||_2,  S = diag(2-norms of the piece's columns of the effective Jacobian).
                 Invariant under column scaling, as a Cholesky solve is.
    covariance   e(C) = max_ij |C_ij - H_ij| / sqrt(H_ii H_jj);  stderr: max_i |se_i - sqrt(H_ii)| / sqrt(H_ii)
Rule:
    e_dev <= 16 * max(e_ref, max(16, k) * 2^-53),  k = unknowns of the piece
e_ref is the same metric for fp64 numpy / LAPACK on the same fp64 operand.  The factor 16 is the one
test_e_gpu_blockqr.py::test_ill_conditioned_blocks uses (another summation order, reciprocals good to 1 ulp); the floor keeps
a case from failing because LAPACK happened to be exact: k roundings are the natural unit of a length-k accumulation.  The
bound comes from the reference and that factor, never from what the code under test returns.

Operand families (each built per block from a seeded generator):
    plain    the library generator, N(0,1)/sqrt(mb); damping 0.05 + U(0,1)
    graded   plain, column j times 10^(-8 j/(k-1)) across the locals and then the shared columns (an amplitude / rate Jacobian);
             damping 0.1 * colsumabs2, which is what LevenbergMarquardt forms.  Also as a column-scaled handle: V plain, s graded
    ill      U diag(logspace(0, -3, k)) V': cond(G) = 1e6; damping 1e-9 * colsumabs2, or none
    far+/-   plain with operand and y times 2^100 / 2^-100 (damping times 2^200 / 2^-200: the same x)
"""
import numpy as np

import hp_reference as hp
import lsq_amd as lsq

LD = hp.LD
FACTOR = 16.0
UNIT = 2.0 ** -53
FAMILIES = ("plain", "graded", "ill", "far+", "far-")
BD_B, BD_MB = 7, 70             # the block-diagonal cases: a grid that ends inside a workgroup of four, two chunks and a ragged third
BD_NBS = (5, 16, 17, 33, 48, 64)


def bd_seed(nb):
    return 100 * nb + 77


# ------------------------------------------------------------------------------------------ the rule
def bound(e_ref, k):
    return FACTOR * max(float(e_ref), max(16, k) * UNIT)


def accepted(e_dev, e_ref, k):
    return bool(np.isfinite(e_dev)) and float(e_dev) <= bound(e_ref, k)


def judge(label, pieces):
    """pieces: (name, e_dev, e_ref, k).  Prints the piece closest to (or furthest beyond) its bound, asserts every piece."""
    assert pieces
    worst = max(pieces, key=lambda p: (float(p[1]) / bound(p[2], p[3])) if np.isfinite(p[1]) else np.inf)
    name, e_dev, e_ref, k = worst
    print("ACC %s | %d pieces | worst %s: e_dev %.3e e_ref %.3e ratio %.2f bound %.3e"
          % (label, len(pieces), name, e_dev, e_ref, float(e_dev) / max(float(e_ref), 1e-300), bound(e_ref, k)))
    bad = [(n, float(d), float(r), k_) for n, d, r, k_ in pieces if not accepted(d, r, k_)]
    assert not bad, (label, bad[:4])


# ------------------------------------------------------------------------------------------ the metrics
def colnorms(A):
    A = hp.ld(A)
    return np.sqrt(np.sum(A * A, axis=0))


def solve_err(x, x_hp, S):
    x, x_hp = hp.ld(x), hp.ld(x_hp)
    d = S * (x - x_hp)
    r = S * x_hp
    return float(np.sqrt(d @ d) / np.sqrt(r @ r))


def cov_err(Cm, H):
    Cm, H = hp.ld(Cm), hp.ld(H)
    sd = np.sqrt(np.diag(H))
    return float(np.max(np.abs(Cm - H) / np.outer(sd, sd)))


def stderr_err(se, H):
    sd = np.sqrt(np.diag(hp.ld(H)))
    return float(np.max(np.abs(hp.ld(se) - sd) / sd))


def s2_of(f, dof):
    f = hp.ld(f)
    return (f @ f) / LD(dof)


# ------------------------------------------------------------------------------------------ operands
class Operand:
    """J: the effective Jacobian in fp64 (a container or an array); y; damp: the family's LM damping; V, s: the same operand
    as a column-scaled handle (graded only: J = fl(V diag(s)), the handle itself computes with V diag(s))."""

    def __init__(self, J, y, damp, V=None, s=None):
        self.J, self.y, self.damp, self.V, self.s = J, y, damp, V, s


def grading(k, decades=8.0):
    return 10.0 ** (-decades * np.arange(k) / (k - 1))


def ill_matrix(rng, m, k, decades=3.0):
    U, _ = np.linalg.qr(rng.standard_normal((m, k)))
    V, _ = np.linalg.qr(rng.standard_normal((k, k)))
    return (U * np.logspace(0, -decades, k)) @ V.T


def colsumabs2(J):
    if isinstance(J, np.ndarray):
        return np.sum(J * J, axis=0)
    B, mb, nb = J.nblocks, J.mb, J.nb
    loc = np.sum(J.data[:B * mb * nb].reshape((B * nb, mb)) ** 2, axis=1)
    if hasattr(J, "border"):
        return np.concatenate([loc, np.sum(J.border ** 2, axis=0)])
    return loc


def _finish(family, J, V, s, rng, m, n, make):
    """y, the family's damping, the far scaling; make(data) builds the container around a value array."""
    y = rng.standard_normal(m)
    if family in ("plain", "far+", "far-"):
        damp = 0.05 + rng.random(n)
        if family != "plain":
            f = 2.0 ** (100 if family == "far+" else -100)
            J, y, damp = make(J.data * f), y * f, damp * f * f
        return Operand(J, y, damp)
    if family == "graded":
        return Operand(J, y, 0.1 * colsumabs2(J), V, s)
    assert family == "ill"
    return Operand(J, y, 1e-9 * colsumabs2(J))


def bd_operand(family, B, mb, nb, seed):
    rng = np.random.default_rng(seed)
    make = lambda data: lsq.BlockDiagonal(B, mb, nb, data=data)
    V = s = None
    if family == "ill":
        J = lsq.BlockDiagonal.from_blocks([ill_matrix(rng, mb, nb) for _ in range(B)])
    else:
        J = make(lsq.synthetic.blockdiag_inputs(B, mb, nb, seed))
        if family == "graded":
            V, s = J, np.tile(grading(nb), B)
            J = make(V.data * np.repeat(s, mb))
    return _finish(family, J, V, s, rng, B * mb, B * nb, make)


def bb_scale_values(V, s):
    B, mb, nb = V.nblocks, V.mb, V.nb
    return V.data * np.concatenate([np.repeat(s[:B * nb], mb), np.repeat(s[B * nb:], B * mb)])


def bb_operand(family, B, mb, nb, ng, seed):
    rng = np.random.default_rng(seed)
    make = lambda data: lsq.BorderedBlockDiagonal(B, mb, nb, ng, data=data)
    V = s = None
    if family == "ill":
        pieces = [ill_matrix(rng, mb, nb + ng) for _ in range(B)]
        J = lsq.BorderedBlockDiagonal.from_blocks([p[:, :nb] for p in pieces], np.vstack([p[:, nb:] for p in pieces]))
    else:
        J = make(lsq.synthetic.bordered_inputs(B, mb, nb, ng, seed))
        if family == "graded":
            g = grading(nb + ng)
            V, s = J, np.concatenate([np.tile(g[:nb], B), g[nb:]])
            J = make(bb_scale_values(V, s))
    return _finish(family, J, V, s, rng, B * mb, B * nb + ng, make)


def dense_operand(family, m, n, seed):
    rng = np.random.default_rng(seed)
    if family == "ill":
        D = ill_matrix(rng, m, n)
    else:
        D = lsq.synthetic.dense_inputs(m, n, seed).reshape((m, n), order="F")
        if family == "graded":
            D = D * grading(n)
    y = rng.standard_normal(m)
    cs = np.sum(D * D, axis=0)
    damp = {"plain": 0.05 + rng.random(n), "graded": 0.1 * cs, "ill": 1e-9 * cs}[family]
    return Operand(np.asfortranarray(D), y, damp)


# ------------------------------------------------------------------------------------------ longdouble and fp64 references
def bd_effective(op, b, scaled_handle=False):
    """Block b of the effective Jacobian in longdouble: fl(V diag(s)) as stored, or V diag(s) unrounded for the scaled handle."""
    if scaled_handle:
        nb = op.V.nb
        return hp.ld(op.V.block(b)) * hp.ld(op.s[b * nb:(b + 1) * nb])
    return hp.ld(op.J.block(b))


def bd_solve_pieces(op, x, damp, scaled_handle=False):
    """(name, e_dev, e_ref, k) per block of a block-diagonal solve; e_ref: numpy.linalg.solve on the fp64 normal equations."""
    J = op.J
    B, mb, nb = J.nblocks, J.mb, J.nb
    out = []
    for b in range(B):
        A = bd_effective(op, b, scaled_handle)
        yb = op.y[b * mb:(b + 1) * mb]
        db = None if damp is None else damp[b * nb:(b + 1) * nb]
        x_hp = hp.normal_solve(A, yb, db)
        A64 = J.block(b)
        G = A64.T @ A64
        if db is not None:
            G = G + np.diag(db)
        x_ref = np.linalg.solve(G, A64.T @ yb)
        S = colnorms(A)
        out.append(("block %d" % b, solve_err(x[b * nb:(b + 1) * nb], x_hp, S), solve_err(x_ref, x_hp, S), nb))
    return out


DENSE_REF_MAX_N = 2048          # tests/test_f_gpu_bordered.py::dense_solve: beyond it the fp64 reference eliminates by blocks


def bb_fp64_solve(J, y, damp):
    if J.shape[1] <= DENSE_REF_MAX_N:
        D = J.toarray()
        return np.linalg.solve(D.T @ D + np.diag(damp), D.T @ y)
    B, mb, nb, ng = J.nblocks, J.mb, J.nb, J.ng
    S = J.border.T @ J.border + np.diag(damp[B * nb:])
    rg = J.border.T @ y
    keep = []
    for b in range(B):
        A, Cb, yb = J.block(b), J.border_block(b), y[b * mb:(b + 1) * mb]
        G = A.T @ A + np.diag(damp[b * nb:(b + 1) * nb])
        W = np.linalg.solve(G, np.column_stack([A.T @ Cb, A.T @ yb]))
        S -= (A.T @ Cb).T @ W[:, :ng]
        rg -= (A.T @ Cb).T @ W[:, ng]
        keep.append(W)
    xg = np.linalg.solve(S, rg)
    return np.concatenate([W[:, ng] - W[:, :ng] @ xg for W in keep] + [xg])


def bb_colnorms(op, scaled_handle=False):
    J = op.J
    B, mb, nb = J.nblocks, J.mb, J.nb
    if scaled_handle:
        V, s = op.V, hp.ld(op.s)
        loc = [colnorms(hp.ld(V.block(b)) * s[b * nb:(b + 1) * nb]) for b in range(B)]
        return loc, colnorms(hp.ld(V.border) * s[B * nb:])
    return [colnorms(J.block(b)) for b in range(B)], colnorms(J.border)


def bb_solve_pieces(op, x, damp, scaled_handle=False):
    J = op.J
    B, nb, ng = J.nblocks, J.nb, J.ng
    if scaled_handle:
        x_hp = hp.arrowhead_solve(op.V, op.y, damp, colscale=op.s)
    else:
        x_hp = hp.arrowhead_solve(J, op.y, damp)
    x_ref = bb_fp64_solve(J, op.y, np.zeros(J.shape[1]) if damp is None else damp)
    loc, sh = bb_colnorms(op, scaled_handle)
    out = []
    for b in range(B):
        sl = slice(b * nb, (b + 1) * nb)
        out.append(("block %d" % b, solve_err(x[sl], x_hp[sl], loc[b]), solve_err(x_ref[sl], x_hp[sl], loc[b]), nb))
    sl = slice(B * nb, B * nb + ng)
    out.append(("shared", solve_err(x[sl], x_hp[sl], sh), solve_err(x_ref[sl], x_hp[sl], sh), ng))
    return out


def cov_pieces(name, Cdev, se_dev, Cref, H, k):
    """The covariance piece and its stderr piece against H (longdouble, already times s^2); Cref: fp64 numpy, times s^2."""
    return [(name, cov_err(Cdev, H), cov_err(Cref, H), k),
            (name + " stderr", stderr_err(se_dev, H), stderr_err(np.sqrt(np.diag(Cref)), H), k)]


# ------------------------------------------------------------------------------------------ fp64 stand-in of the device algorithm
def standin_gram(A):
    """A'A accumulated over 32-row chunks, every chunk's sum over its rows split four ways (rows q, q + 4, ..), in fp64."""
    m, n = A.shape
    G = np.zeros((n, n))
    for c in range(0, m, 32):
        ch = A[c:c + 32]
        for q in range(4):
            G = G + ch[q::4].T @ ch[q::4]
    return G


def _rsqrt(a, degraded):
    r = 1.0 / np.sqrt(a)
    return np.float64(np.float32(r)) if degraded else r


def standin_factor(G, degraded=False):
    """Right-looking Cholesky G = U'U that MULTIPLIES by a reciprocal square root.  degraded: that reciprocal square root is
    rounded through float32 (the hardware estimate's 2^-24) and not corrected."""
    M = np.array(G, dtype=np.float64)
    n = M.shape[0]
    U = np.zeros((n, n))
    for j in range(n):
        row = M[j, j:] * _rsqrt(M[j, j], degraded)
        U[j, j:] = row
        M[j + 1:, j + 1:] -= np.outer(row[1:], row[1:])
    return U


def _tri_solves(U, r):
    n = U.shape[0]
    z = np.array(r, dtype=np.float64)
    dinv = 1.0 / np.diag(U)
    for k in range(n):
        z[k] = z[k] * dinv[k]
        z[k + 1:] -= U[k, k + 1:] * z[k]
    for k in range(n - 1, -1, -1):
        z[k] = z[k] * dinv[k]
        z[:k] -= U[:k, k] * z[k]
    return z


def standin_solve(A, y, damp=None, degraded=False):
    G = standin_gram(A)
    if damp is not None:
        G = G + np.diag(damp)
    return _tri_solves(standin_factor(G, degraded), A.T @ y)


def standin_inv(A, degraded=False):
    U = standin_factor(standin_gram(A), degraded)
    n = U.shape[0]
    X = np.zeros((n, n))
    dinv = 1.0 / np.diag(U)
    for r in range(n - 1, -1, -1):                    # inv(U) by back substitution, a reciprocal per pivot
        e = np.zeros(n)
        e[r] = 1.0
        X[r] = (e - U[r, r + 1:] @ X[r + 1:]) * dinv[r]
    return X @ X.T
