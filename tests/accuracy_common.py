"""The accuracy tier's operands, metrics and acceptance rule, shared by tests/test_accuracy_host.py (no device),
tests/test_h_gpu_accuracy.py and tests/test_i_gpu_accuracy_*.py.  The reference is tests/hp_reference.py (numpy.longdouble).

Metrics -- all in longdouble, per PIECE (each block; the shared part of a bordered handle separately), so that a small piece
cannot hide inside a large one:
    solve        e(x) = ||S (x - x_hp)||_2 / ||S x_hp||_2,  S = diag(2-norms of the piece's columns of the effective Jacobian).
                 Invariant under column scaling, as a Cholesky solve is.
    covariance   e(C) = max_ij |C_ij - H_ij| / sqrt(H_ii H_jj);  stderr: max_i |se_i - sqrt(H_ii)| / sqrt(H_ii)
Rule:
    e_dev <= 16 * max(e_ref, min(max(16, k), 64) * 2^-53),  k = unknowns of the piece
e_ref is the same metric for fp64 numpy / LAPACK on the same fp64 operand.  The factor 16 is the one
test_e_gpu_blockqr.py::test_ill_conditioned_blocks uses (another summation order, reciprocals good to 1 ulp); the floor keeps
a case from failing because LAPACK happened to be exact: k roundings are the natural unit of a length-k accumulation -- of a
small piece.  A normwise error over hundreds of unknowns averages, it does not add up (LAPACK's Householder QR stays at 1e-15
at k = 321), so the floor stops growing at k = 64, the widest piece the block solvers have.  The bound comes from the
reference and that factor, never from what the code under test returns.

Products (product_bound): every output element i of alpha * A x + beta * y must lie within
    gamma_(K_i + c) * (|alpha| sum_k |a_ik x_k| + |beta y_i|),   gamma_t = t u / (1 - t u),  u = 2^-53
of the longdouble value: the standard bound of a length-K_i dot product in ANY summation order, with or without FMA
(Higham, Accuracy and Stability of Numerical Algorithms, section 3.1), K_i the stored entries that contribute, c <= 8 the further
roundings counted from the kernel's code.

Operand families (each built per block from a seeded generator):
    plain    the library generator, N(0,1)/sqrt(mb); damping 0.05 + U(0,1)
    graded   plain, column j times 10^(-8 j/(k-1)) across the locals and then the shared columns (an amplitude / rate Jacobian);
             damping 0.1 * colsumabs2, which is what LevenbergMarquardt forms.  Also as a column-scaled handle: V plain, s graded
    ill      U diag(logspace(0, -3, k)) V': cond(G) = 1e6; damping 1e-9 * colsumabs2, or none
    far+/-   plain with operand and y times 2^100 / 2^-100 (damping times 2^200 / 2^-200: the same x)

Dense operands come with two right-hand sides.  random: y standard normal -- a large residual, whose term
cond^2 u ||r|| / (||A|| ||x||) enters the error of EVERY least-squares solver, a backward-stable QR included.  consistent:
y = fl(A (z / colnorms)), z standard normal -- a residual at rounding level, where a QR has cond u and anything that squares
the condition number still cond^2 u: the sharper of the two (tests/test_accuracy_host.py: the fp64 normal equations are 36 to
41 x beyond the bound there, 19 to 20 x on the random y).
"""
import functools

import numpy as np

import hp_reference as hp
import lsq_amd as lsq

LD = hp.LD
FACTOR = 16.0
UNIT = 2.0 ** -53
FLOOR_CAP = 64                  # the floor max(16, k) 2^-53 stops growing here
FAMILIES = ("plain", "graded", "ill", "far+", "far-")
BD_B, BD_MB = 7, 70             # the block-diagonal cases: a grid that ends inside a workgroup of four, two chunks and a ragged third
BD_NBS = (5, 16, 17, 33, 48, 64)


def bd_seed(nb):
    return 100 * nb + 77


# ------------------------------------------------------------------------------------------ the rule
def bound(e_ref, k):
    return FACTOR * max(float(e_ref), min(max(16, k), FLOOR_CAP) * UNIT)


def lsmr_bound(e_ref, n, iters):
    """The same rule for an LSMR iterate after `iters` iterations (tests/test_k_gpu_lsmr_stops.py): the floor is scaled by the
    iteration count, because every iteration adds a product's worth of rounding to the recurrence."""
    return FACTOR * max(float(e_ref), min(max(16, n), FLOOR_CAP) * UNIT * iters)


def trajectory_bound(e_ref, k, iteration, cond=1.0):
    """The same rule for a quantity of outer iteration `iteration` (counted from 1) of a trust-region run
    (tests/test_v_gpu_trust_region.py): the floor is that of a sum of length k, once per iteration the run has behind it, times
    `cond`, the condition number of the quantity with respect to those sums where it is not 1 (rho: ssr / pred_red, the
    quotient of two differences of sums of squares; the gradient norm: max |J|'|f| / max |J'f|)."""
    return FACTOR * max(float(e_ref), min(max(16, k), FLOOR_CAP) * UNIT * iteration * max(1.0, float(cond)))


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


def dense_operand(family, m, n, seed, rhs="random"):
    """rhs: "random" or "consistent" (the module docstring); the operand and its damping do not depend on it."""
    assert rhs in ("random", "consistent")
    rng = np.random.default_rng(seed)
    if family == "ill":
        D = ill_matrix(rng, m, n)
    else:
        D = lsq.synthetic.dense_inputs(m, n, seed).reshape((m, n), order="F")
        if family == "graded":
            D = D * grading(n)
    y = rng.standard_normal(m)
    cs = np.sum(D * D, axis=0)
    damp = (0.1 * cs) if family == "graded" else (1e-9 * cs) if family == "ill" else 0.05 + rng.random(n)
    if rhs == "consistent":         # (drawn after everything else: the random operand is the one it always was)
        y = D @ (rng.standard_normal(n) / np.sqrt(cs))
    if family in ("far+", "far-"):
        f = 2.0 ** (100 if family == "far+" else -100)
        D, y, damp = D * f, y * f, damp * f * f
    return Operand(np.asfortranarray(D), y, damp)


def stacked(A, y, damp):
    """[A; diag(sqrt(damp))] and [y; 0] (y a vector or a matrix of right-hand sides), in the dtype of A: the least-squares
    problem whose normal equations are the damped ones."""
    n = A.shape[1]
    zeros = np.zeros((n,) + np.shape(y)[1:], dtype=A.dtype)
    return np.vstack([A, np.diag(np.sqrt(np.asarray(damp).astype(A.dtype)))]), np.concatenate([np.asarray(y).astype(A.dtype), zeros])


def qr_fp64_solve(A, y):
    """min ||A x - y|| by LAPACK's Householder QR (numpy.linalg.qr) and one triangular solve, all in fp64.  On graded
    columns it is two to three orders closer to the longdouble solution than numpy.linalg.lstsq (gelsd: an SVD, not invariant
    under column scaling), so it is the e_ref of the QR cases."""
    Q, R = np.linalg.qr(A)
    return np.linalg.solve(R, Q.T @ y)


# ------------------------------------------------------------------------------------------ the dense QR cases and their references
RHS = ("random", "consistent")
QR_PANEL_SHAPES = [(640, 128), (700, 130), (1000, 321), (400, 256)]
QR_PANEL_FAMILIES = ("plain", "graded", "ill")
QR_ROW_VARIANT_MS, QR_ROW_VARIANT_N = [3000, 6000, 12000, 22000], 70
QR_TSQR_SHAPES = [(33000, 8), (40000, 12), (36000, 16), (40000, 20), (34000, 24), (33000, 28), (40000, 31), (140000, 31)]
QR_TSQR_FAMILIES = ("plain", "graded", "far+", "far-")


def cases(shapes, families):
    """(m, n, family, rhs, damped), the operand varying slowest: consecutive cases share one cached reference."""
    return [(m, n, f, r, d) for (m, n) in shapes for f in families for r in RHS for d in (False, True)]


def dense_seed(m, n):
    return 9000 + m + n


class QrRef:
    """One dense operand with both right-hand sides, its longdouble solutions (undamped and damped, computed on first use, one
    factorisation for both right-hand sides) and the fp64 Householder QR's error on each of the four problems.  far+ / far-
    take plain's x_hp: scaling operand and y by 2^100 (damping by 2^200) changes no bit of any quotient
    (tests/test_accuracy_host.py::test_far_operand_has_the_bits_of_plain)."""

    def __init__(self, family, m, n):
        ops = [dense_operand(family, m, n, dense_seed(m, n), rhs) for rhs in RHS]
        assert np.array_equal(ops[0].J, ops[1].J)
        self.family, self.m, self.n = family, m, n
        self.A, self.damp = ops[0].J, ops[0].damp
        self.Y = np.column_stack([ops[0].y, ops[1].y])
        self.S = colnorms(self.A)
        self._x_hp, self._e_ref = {}, {}

    def problem(self, rhs, damped):
        """The fp64 least-squares problem of the case: (A, y), stacked if damped."""
        y = self.Y[:, RHS.index(rhs)]
        return stacked(self.A, y, self.damp) if damped else (self.A, y)

    def x_hp(self, rhs, damped):
        if damped not in self._x_hp:
            if self.family in ("far+", "far-"):
                self._x_hp[damped] = qr_ref("plain", self.m, self.n).x_hp(None, damped)
            else:
                A, Y = hp.ld(self.A), hp.ld(self.Y)
                if damped:
                    A, Y = stacked(A, Y, self.damp)
                self._x_hp[damped] = hp.lstsq_qr(A, Y)
        X = self._x_hp[damped]
        return X if rhs is None else X[:, RHS.index(rhs)]

    def err(self, x, rhs, damped):
        return solve_err(x, self.x_hp(rhs, damped), self.S)

    def e_ref(self, rhs, damped):
        if (rhs, damped) not in self._e_ref:
            self._e_ref[rhs, damped] = self.err(qr_fp64_solve(*self.problem(rhs, damped)), rhs, damped)
        return self._e_ref[rhs, damped]


@functools.lru_cache(maxsize=6)
def qr_ref(family, m, n):
    return QrRef(family, m, n)


# ------------------------------------------------------------------------------------------ products, per output element
def gamma(t):
    t = hp.ld(t)
    return t * LD(UNIT) / (1 - t * LD(UNIT))


def product_reference(A, x, alpha, beta, y):
    """(ref, mag) of alpha * A x + beta * y per output element in longdouble; mag = |alpha| sum_k |a_ik x_k| + |beta y_i|.
    A: a dense longdouble copy of the effective operand (zeros where nothing is stored)."""
    A, x, y = hp.ld(A), hp.ld(x), hp.ld(y)
    a, b = LD(alpha), LD(beta)
    return a * (A @ x) + b * y, abs(a) * (np.abs(A) @ np.abs(x)) + np.abs(b * y)


def product_bound(K, c, mag):
    """gamma_(K_i + c) * mag_i; K: stored entries per output, c: further roundings (at most 8)."""
    assert 0 <= c <= 8
    return gamma(np.asarray(K) + c) * mag


def product_excess(out, ref, K, c, mag):
    """max_i |out_i - ref_i| / bound_i over the outputs with a nonzero bound (elsewhere out must equal ref), and its index."""
    d = np.abs(hp.ld(out) - ref)
    b = product_bound(K, c, mag)
    zero = b == 0
    if np.any(d[zero] != 0) or not np.all(np.isfinite(d.astype(float))):
        return np.inf, int(np.argmax(np.where(zero, d, 0)))
    q = np.where(zero, 0, d / np.where(zero, 1, b))
    i = int(np.argmax(q))
    return float(q[i]), i


def judge_product(label, out, ref, K, c, mag):
    q, i = product_excess(out, ref, K, c, mag)
    print("ACC product %s | %d outputs | worst %d: |err| / bound %.3f (K %d, bound %.3e)"
          % (label, len(ref), i, q, int(np.asarray(K)[i]), float(product_bound(K, c, mag)[i])))
    assert q <= 1.0, (label, i, q)


def ragged_pattern(m, n, density, seed):
    """The pattern of tests/test_b_gpu_kernels.py::test_sparse_products: random, one full row (5), an empty column (1) and an
    empty row (3).  scipy CSC with sorted indices."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    S = sp.random(m, n, density=density, format="lil", random_state=rng, data_rvs=rng.standard_normal)
    S[5, :] = rng.standard_normal(n)
    S[:, 1] = 0
    S[3, :] = 0
    S = S.tocsc()
    S.sort_indices()
    S.eliminate_zeros()
    return S


def product_scales(m, n, seed):
    """r (m) and c (n): 12 decades each, shuffled, so that neighbours in a slice, a window or a wavefront differ in scale."""
    rng = np.random.default_rng(seed)
    return rng.permutation(grading(m, 12.0)), rng.permutation(grading(n, 12.0))


def product_vectors(r, c, seed):
    """The vectors of the two products of diag(r) S diag(c), balanced so that EVERY stored entry matters to its output and the
    beta term hides none: J x gets x = z / c (all terms of a row are of the row's size r_i) and is added to y = r * z';
    J'y gets y = z' / r and is added to x = c * z.  Returns ((x, y) of J x, (y, x) of J'y): (factor, addend) each."""
    rng = np.random.default_rng(seed)
    z, zz = rng.standard_normal((2, len(c)))
    w, ww = rng.standard_normal((2, len(r)))
    return (z / c, r * w), (ww / r, c * zz)


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
