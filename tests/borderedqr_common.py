"""Shared by tests/test_borderedqr_host.py (no device) and tests/test_u_gpu_borderedqr.py: the numpy fp64 twin of the
BorderedQR() solver (lsq_borderedqr.hip), the six-decade `ill6` family, and the accuracy rule of the QR cases on a bordered
operand.  The shapes of the solve, accuracy, bits and loop cases are tests/schur_common.py's, unchanged.

The twin follows the device code stage by stage, in fp64.  Per block b, the running triangle starts as diag(sqrt(damp_b)) and
the rows of [J_b | C_b | y_b] are eliminated against it in chunks of H rows (64 when mb > 32, else 32), unpivoted:
    Q_b' [diag(sqrt(damp_b)) 0 0; J_b C_b y_b] = [R_b W_b z_b; 0 F_b r_b]
The stacked F_b, r_b and the last ng damping values are ONE fp64 Householder solve (accuracy_common.qr_fp64_solve) for x_g;
x_b = inv(R_b) (z_b - W_b x_g).

The accuracy rule (accuracy_common.bound, per piece: each block, then the shared part):
    x_hp   hp_reference.lstsq_qr on the stacked dense matrix [J; diag(sqrt(damp))], right-hand side [y; 0], in longdouble
    e_ref  accuracy_common.qr_fp64_solve on the same stacked problem in fp64
Neither comes from the code under test.

ill6: per block accuracy_common.ill_matrix(rng, mb, nb + ng, decades=6.0) split into J_b and C_b, cond(J'J) = 1e12;
damping 1e-14 * colsumabs2; both right-hand sides of accuracy_common's docstring (random / consistent).  The fp64 normal
equations (accuracy_common.bb_fp64_solve) are beyond the bound on every one of these cases, a backward-stable solver is not:
the cases tell the two kinds of solver apart (tests/test_borderedqr_host.py asserts both)."""
import functools

import numpy as np

import accuracy_common as ac
import hp_reference as hp
import lsq_amd as lsq
import schur_common as sc

ILL6_SHAPES = [(5, 96, 5, 3), (5, 96, 16, 48), (3, 160, 17, 65), (3, 96, 64, 32)]     # (B, mb, nb, ng), mb >= nb + ng


def ill6_cases():
    return [(shape, rhs) for shape in ILL6_SHAPES for rhs in ac.RHS]


@functools.lru_cache(maxsize=None)
def ill6_operands(B, mb, nb, ng):
    """{rhs: Operand}: the same J and damping under both right-hand sides."""
    rng = np.random.default_rng(7000 + nb + ng)
    pieces = [ac.ill_matrix(rng, mb, nb + ng, decades=6.0) for _ in range(B)]
    J = lsq.BorderedBlockDiagonal.from_blocks([p[:, :nb] for p in pieces], np.vstack([p[:, nb:] for p in pieces]))
    cs = ac.colsumabs2(J)
    damp = 1e-14 * cs
    y = rng.standard_normal(B * mb)
    yc = J.toarray() @ (rng.standard_normal(B * nb + ng) / np.sqrt(cs))
    return {"random": ac.Operand(J, y, damp), "consistent": ac.Operand(J, yc, damp)}


# ------------------------------------------------------------------------------------------ the twin
def chunk_rows(mb):
    return 64 if mb > 32 else 32


def larfg(alpha, s2):
    """(tau, sc, beta) of bq_larfg: H = I - tau v v', v = (1, x * sc)."""
    if s2 == 0.0:
        return 0.0, 0.0, alpha
    bt = -np.copysign(np.hypot(alpha, np.sqrt(s2)), alpha)
    return (bt - alpha) / bt, 1.0 / (alpha - bt), bt


def eliminate_block(A, Cb, yb, dampb):
    """The triangle-over-rectangle elimination of one block: (R, W, z, F, r, fail); fail: 0, or the 1-based column whose
    diagonal entry of R is zero or not finite (the lowest one)."""
    mb, nb = A.shape
    H = chunk_rows(mb)
    with np.errstate(invalid="ignore"):
        R = np.diag(np.sqrt(np.asarray(dampb, dtype=np.float64)))
    W = np.zeros((nb, Cb.shape[1]))
    z = np.zeros(nb)
    F, r = np.array(Cb, dtype=np.float64), np.array(yb, dtype=np.float64)
    for r0 in range(0, mb, H):
        ch = np.array(A[r0:r0 + H], dtype=np.float64)
        Fc, rc = F[r0:r0 + H], r[r0:r0 + H]                    # views: updated in place
        for j in range(nb):
            x = ch[:, j]
            tau, sc, beta = larfg(R[j, j], x @ x)
            if tau != 0.0:
                v = x * sc
                for M, t in ((ch[:, j + 1:], R[j, j + 1:]), (Fc, W[j])):
                    tw = tau * (v @ M + t)
                    M -= np.outer(v, tw)
                    t -= tw
                tw = tau * (v @ rc + z[j])
                rc -= v * tw
                z[j] -= tw
            R[j, j] = beta
    d = np.abs(np.diag(R))
    bad = np.nonzero(~((d > 0.0) & np.isfinite(d)))[0]
    return R, W, z, F, r, (int(bad[0]) + 1 if len(bad) else 0)


def twin_solve(J, y, damp, colscale=None):
    """J: a BorderedBlockDiagonal; colscale: the handle holds V = J and means V diag(colscale).  Returns (x, 0), or
    (None, column): the 1-based stacked column LSQ_ERANK names (the lowest one)."""
    B, mb, nb, ng = J.nblocks, J.mb, J.nb, J.ng
    s = np.ones(B * nb + ng) if colscale is None else np.asarray(colscale, dtype=np.float64)
    sg = s[B * nb:]
    parts, fail = [], 0
    with np.errstate(all="ignore"):
        for b in range(B):
            sl = slice(b * nb, (b + 1) * nb)
            R, W, z, F, r, bad = eliminate_block(J.block(b) * s[sl], J.border_block(b) * sg, y[b * mb:(b + 1) * mb], damp[sl])
            if bad and not fail:
                fail = b * nb + bad
            parts.append((R, W, z, F, r))
    if fail:
        return None, fail
    Fs, rs = ac.stacked(np.vstack([p[3] for p in parts]), np.concatenate([p[4] for p in parts]), damp[B * nb:])
    xg = ac.qr_fp64_solve(Fs, rs)
    xb = [np.linalg.solve(R, z - W @ xg) for R, W, z, _, _ in parts]
    return np.concatenate(xb + [xg]), 0


# ------------------------------------------------------------------------------------------ the rule
def stacked_dense(J, y, damp):
    """([J; diag(sqrt(damp))], [y; 0]) of a BorderedBlockDiagonal as dense fp64 arrays."""
    return ac.stacked(J.toarray(), y, damp)


def qr_fp64_reference(J, y, damp):
    """The fp64 Householder solve of the stacked dense problem: the reference of the branch tests and e_ref's solver."""
    return ac.qr_fp64_solve(*stacked_dense(J, y, damp))


DENSE_QR_MAX_N = 700            # beyond it the fp64 Householder reference works block by block


def qr_fp64_solve_any(J, y, damp):
    """qr_fp64_reference where the dense stacked matrix is small; else the same Householder solve by LAPACK block by block
    (numpy.linalg.qr of [diag(sqrt(damp_b)); J_b] applied to [0; C_b] and [0; y_b], then the reduced dense problem), the way
    accuracy_common.bb_fp64_solve eliminates by blocks beyond its own limit."""
    if J.shape[1] <= DENSE_QR_MAX_N:
        return qr_fp64_reference(J, y, damp)
    B, mb, nb, ng = J.nblocks, J.mb, J.nb, J.ng
    keep, Fs, rs = [], [], []
    for b in range(B):
        top = np.diag(np.sqrt(damp[b * nb:(b + 1) * nb]))
        Q, R = np.linalg.qr(np.vstack([top, J.block(b)]), mode="complete")
        T = Q.T @ np.vstack([np.zeros((nb, ng + 1)), np.column_stack([J.border_block(b), y[b * mb:(b + 1) * mb]])])
        keep.append((R[:nb], T[:nb, :ng], T[:nb, ng]))
        Fs.append(T[nb:, :ng])
        rs.append(T[nb:, ng])
    xg = ac.qr_fp64_solve(*ac.stacked(np.vstack(Fs), np.concatenate(rs), damp[B * nb:]))
    return np.concatenate([np.linalg.solve(R, z - W @ xg) for R, W, z in keep] + [xg])


class QrPieces:
    """One bordered operand (J, damp; several right-hand sides) with its longdouble solution and the fp64 Householder QR's
    error, computed once.  scaled: the effective Jacobian is V diag(s) unrounded (the column-scaled handle), the fp64
    comparator still works on J = fl(V diag(s))."""

    def __init__(self, op, damp, Y, scaled=False):
        J = op.J
        self.B, self.nb, self.ng = J.nblocks, J.nb, J.ng
        Y = np.asarray(Y, dtype=np.float64).reshape(J.shape[0], -1)
        E = (hp.ld(op.V.toarray()) * hp.ld(op.s)) if scaled else hp.ld(J.toarray())
        As, Ys = ac.stacked(E, hp.ld(Y), damp)
        self.x_hp = hp.lstsq_qr(As, Ys)
        self.x_ref = np.column_stack([qr_fp64_reference(J, Y[:, i], damp) for i in range(Y.shape[1])])
        self.loc, self.sh = ac.bb_colnorms(op, scaled)

    def pieces(self, x, col=0):
        """(name, e_dev, e_ref, k) per block and for the shared part, for right-hand side `col`."""
        B, nb, ng = self.B, self.nb, self.ng
        x_hp, x_ref = self.x_hp[:, col], self.x_ref[:, col]
        out = []
        for b in range(B):
            sl = slice(b * nb, (b + 1) * nb)
            out.append(("block %d" % b, ac.solve_err(x[sl], x_hp[sl], self.loc[b]), ac.solve_err(x_ref[sl], x_hp[sl], self.loc[b]), nb))
        sl = slice(B * nb, B * nb + ng)
        out.append(("shared", ac.solve_err(x[sl], x_hp[sl], self.sh), ac.solve_err(x_ref[sl], x_hp[sl], self.sh), ng))
        return out


    def distance(self, xa, xb, col=0):
        """||S (xa - xb)|| / ||S x_hp|| per piece: by the triangle inequality at most e(xa) + e(xb)."""
        B, nb, ng = self.B, self.nb, self.ng
        x_hp, d = self.x_hp[:, col], hp.ld(xa) - hp.ld(xb)
        sls = [slice(b * nb, (b + 1) * nb) for b in range(B)] + [slice(B * nb, B * nb + ng)]
        return [ac.solve_err(x_hp[sl] + d[sl], x_hp[sl], S) for sl, S in zip(sls, self.loc + [self.sh])]


@functools.lru_cache(maxsize=None)
def acc_reference(family, shape, zero_damping=False, scaled=False):
    """(op, damp, QrPieces) of one case of schur_common.acc_cases(); zero_damping: the `ill` family once more without damping."""
    B, mb, nb, ng = shape
    op = ac.bb_operand(family, B, mb, nb, ng, sc.acc_seed(B, nb, ng))
    damp = np.zeros(B * nb + ng) if zero_damping else op.damp
    return op, damp, QrPieces(op, damp, op.y, scaled)


@functools.lru_cache(maxsize=None)
def ill6_reference(shape):
    """({rhs: Operand}, QrPieces with one column per right-hand side, in the order of accuracy_common.RHS)."""
    ops = ill6_operands(*shape)
    first = ops[ac.RHS[0]]
    return ops, QrPieces(first, first.damp, np.column_stack([ops[r].y for r in ac.RHS]))


def beyond(pieces):
    """The largest e / bound over the pieces: > 1 means outside the rule."""
    return max((float(d) / ac.bound(r, k)) if np.isfinite(d) else np.inf for _, d, r, k in pieces)


# ------------------------------------------------------------------------------------------ failures
def rank_case(name):
    """(J, y, damp, expected 1-based stacked column or 0) on a (4, 20, 3, 5) operand of the library generator.
    zero: column 1 of block 2 is zero and so is its damping value -> column 2 * 3 + 2;  two: the same in blocks 3 and 1 -> the
    lower one, 1 * 3 + 3;  nan: a NaN in column 0 of block 1 -> 1 * 3 + 1;  damped: the zero column of `zero` with its damping
    value left positive -> a solve."""
    B, mb, nb, ng = 4, 20, 3, 5
    J = lsq.BorderedBlockDiagonal(B, mb, nb, ng, data=lsq.synthetic.bordered_inputs(B, mb, nb, ng, 11))
    rng = np.random.default_rng(12)
    y, damp = rng.standard_normal(B * mb), 0.05 + rng.random(B * nb + ng)
    expect = 0
    if name in ("zero", "damped"):
        J.block(2)[:, 1] = 0.0
        if name == "zero":
            damp[2 * nb + 1] = 0.0
            expect = 2 * nb + 2
    elif name == "two":
        J.block(3)[:, 0] = 0.0
        J.block(1)[:, 2] = 0.0
        damp[3 * nb + 0] = damp[1 * nb + 2] = 0.0
        expect = 1 * nb + 3
    elif name == "nan":
        J.block(1)[7, 0] = np.nan
        expect = 1 * nb + 1
    else:
        assert name == "good"
    return J, y, damp, expect


RANK_CASES = ("zero", "two", "nan")
ERANK_TEXT = ("RankDeficientException: BorderedQR(): the triangular factor of the local columns has a zero or non-finite "
              "diagonal entry at column %d (a zero damping value on a zero column, or a non-finite operand)")


# ------------------------------------------------------------------------------------------ a graded global fit
class GradedTanhFit(sc.TanhFit):
    """schur_common.TanhFit with graded features: column j of the local features P and of the shared features Q is scaled by
    10^(-DECADES j / (k - 1)) and the true weight by the inverse, so every parameter matters as much as in the plain fit while
    cond(J) grows by 10^DECADES (an amplitude / rate Jacobian).  DECADES = 4 keeps colsumabs2 inside LevenbergMarquardt's
    clamp [1e-6, 1e32] * mean but for the last few columns, so the damped steps stay (nearly) those of the plain fit."""
    DECADES = 4.0

    def __init__(self, B, mb, nb, ng, seed=42):
        super().__init__(B, mb, nb, ng, seed)
        rng = np.random.default_rng(seed + 1)
        sp, sq = ac.grading(max(nb, 2), self.DECADES)[:nb], ac.grading(max(ng, 2), self.DECADES)[:ng]
        self.P = self.P * sp
        self.Q = self.Q * sq
        truth = np.concatenate([np.tile(1.0 / sp, B) * 0.5 * rng.standard_normal(B * nb), 0.5 * rng.standard_normal(ng) / sq])
        self.sigma = 1e-3
        self.data = np.tanh(self.arg(truth)) + self.sigma * rng.standard_normal(self.m)
