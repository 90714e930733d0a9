"""Shared by tests/test_schur_host.py (no device) and tests/test_r_gpu_schur.py: the case lists of the Schur() solver
(lsq_schur.hip), its numpy fp64 twin, the operands whose failing pivot is exact, and the global tanh fit of the loop tests.

The twin follows the five steps of the device code, in fp64, block by block.  With U_bb'U_bb = J_b'J_b + D_b:
    W_b = inv(U_bb)' J_b'C_b        z_b = inv(U_bb)' J_b'y_b
    S   = C'C + D_g - W'W           r_g = C'y - W'z
    x_g = S \\ r_g (unpivoted Cholesky)        x_b = inv(U_bb) (z_b - W_b x_g)
"""
import numpy as np

import accuracy_common as ac
import lsq_amd as lsq

SOLVE_RTOL = 1e-9        # tests/gpu_common.py: one direct solve (ldiv!), as tests/test_f_gpu_bordered.py uses it

NBS = (1, 5, 16, 17, 33, 64)
NGS = (1, 31, 32, 63, 64, 65, 128, 129, 200)
MBS = (1, 7, 37, 64, 100)
BS = (1, 2, 3, 64, 65, 130)
# (B, mb, nb, ng): every value above with at least two values of every other size (test_schur_host.py checks that).  nb: one
# wavefront per block (1, 5, 16) and one workgroup per block with 2, 3, 4 tile rows; ng: the edges of the 64-column border tile,
# both sides of the inner solver's one-workgroup / blocked switch (31 | 32 at these m) and of its one-launch factorisation (from
# 128), ng no multiple of 16; mb: below one row chunk, mb < nb (the damping makes it solvable), a ragged fourth chunk.
BRANCH_SHAPES = [(1, 1, 1, 1), (65, 7, 5, 31), (3, 37, 16, 32), (1, 64, 17, 63), (65, 100, 33, 64), (3, 1, 64, 65),
                 (130, 7, 1, 128), (64, 37, 5, 129), (2, 64, 16, 200), (130, 100, 17, 1), (64, 1, 33, 31), (2, 7, 64, 32),
                 (65, 37, 1, 63), (3, 64, 5, 64), (1, 100, 16, 65), (65, 1, 17, 128), (3, 7, 33, 129), (1, 37, 64, 200)]
# K of the two tall products (B nb rows of W, m rows of C) on, just above and near a boundary of the 32-row slabs and of the
# split-K slices (multiples of 32 rows): 1024 / 4096, 1040 / 4160, 325 / 2405
SLICE_SHAPES = [(64, 64, 16, 65), (65, 64, 16, 129), (65, 37, 5, 64)]
SOLVE_SHAPES = BRANCH_SHAPES + SLICE_SHAPES
DENSE_HANDLE_MAX = 1500000       # m * n up to which the stacked matrix also goes through lsq_dense_create

# accuracy tier: (B, mb, nb, ng); the last four have nb + ng > 64.  mb >= nb + ng (the "ill" family takes a QR of the augmented
# block), n <= 400 for the longdouble reference.  Seeds: 1000 nb + 10 ng + B, as tests/test_h_gpu_accuracy.py.
ACC_SHAPES = [(5, 96, 5, 3), (5, 96, 16, 48), (5, 96, 40, 24), (5, 96, 5, 70), (5, 96, 17, 65), (5, 96, 33, 63), (3, 96, 64, 32)]
AGREE_SHAPES = [(16, 48), (5, 8), (60, 4)]      # (nb, ng) with nb + ng <= 64: Schur() against Cholesky() on the same handle


def acc_seed(B, nb, ng):
    return 1000 * nb + 10 * ng + B


def acc_cases():
    return [(family, shape) for shape in ACC_SHAPES for family in ac.FAMILIES]


def make_bb(B, mb, nb, ng, seed):
    return lsq.BorderedBlockDiagonal(B, mb, nb, ng, data=lsq.synthetic.bordered_inputs(B, mb, nb, ng, seed))


def solve_operand(B, mb, nb, ng):
    """The library generator's operand, y and a damping in [0.05, 1.05): well conditioned, also where mb < nb."""
    J = make_bb(B, mb, nb, ng, 1000 * nb + 10 * ng + mb + B)
    rng = np.random.default_rng(nb * mb + B + ng)
    return J, rng.standard_normal(B * mb), 0.05 + rng.random(B * nb + ng)


def rel_err(x, ref):
    return np.linalg.norm(x - ref) / np.linalg.norm(ref)


# ------------------------------------------------------------------------------------------ the twin
def chol_upper(G):
    """Right-looking unpivoted Cholesky G = U'U (upper triangle of G is read).  Returns (U, 0), or (None, k): the 1-based column
    whose pivot is not positive."""
    A = np.array(G, dtype=np.float64)
    n = A.shape[0]
    for j in range(n):
        if not A[j, j] > 0.0:
            return None, j + 1
        A[j, j:] = A[j, j:] / np.sqrt(A[j, j])
        if j + 1 < n:
            A[j + 1:, j + 1:] -= np.outer(A[j, j + 1:], A[j, j + 1:])
    return np.triu(A), 0


def forward(U, R):
    """inv(U)' R by substitution."""
    X = np.array(R, dtype=np.float64)
    for k in range(U.shape[0]):
        X[k] = (X[k] - U[:k, k] @ X[:k]) / U[k, k]
    return X


def backward(U, R):
    """inv(U) R by substitution."""
    X = np.array(R, dtype=np.float64)
    for k in range(U.shape[0] - 1, -1, -1):
        X[k] = (X[k] - U[k, k + 1:] @ X[k + 1:]) / U[k, k]
    return X


def twin_solve(J, y, damp, colscale=None):
    """The five steps in fp64.  J: a BorderedBlockDiagonal; colscale: the handle holds V = J and means V diag(colscale).
    Returns (x, 0), or (None, column): the 1-based stacked column of the PosDefException (the lowest one)."""
    B, mb, nb, ng = J.nblocks, J.mb, J.nb, J.ng
    s = np.ones(B * nb + ng) if colscale is None else np.asarray(colscale, dtype=np.float64)
    sg = s[B * nb:]
    C = J.border
    Us, zs, Ws = [], [], []
    fail = 0
    for b in range(B):
        A, Cb, yb = J.block(b), J.border_block(b), y[b * mb:(b + 1) * mb]
        sb = s[b * nb:(b + 1) * nb]
        G = (A.T @ A) * np.outer(sb, sb) + np.diag(damp[b * nb:(b + 1) * nb])
        U, bad = chol_upper(G)
        if bad:
            fail = fail or b * nb + bad
            U = np.eye(nb)
        Us.append(U)
        zs.append(forward(U, (A.T @ yb) * sb))
        Ws.append(forward(U, (A.T @ Cb) * np.outer(sb, sg)))
    W, z = np.vstack(Ws), np.concatenate(zs)
    S = (C.T @ C) * np.outer(sg, sg) - W.T @ W + np.diag(damp[B * nb:])
    rg = (C.T @ y) * sg - W.T @ z
    Ug, bad = chol_upper(S)
    if fail or bad:
        return None, fail or B * nb + bad
    xg = backward(Ug, forward(Ug, rg))
    xb = [backward(Us[b], zs[b] - Ws[b] @ xg) for b in range(B)]
    return np.concatenate(xb + [xg]), 0


def stacked_potrf_column(J, damp):
    """0, or the 1-based column at which the unpivoted Cholesky of the dense stacked normal matrix stops."""
    D = J.toarray()
    return chol_upper(D.T @ D + np.diag(damp))[1]


# ------------------------------------------------------------------------------------------ exact failures
def exact_operand(B, nb, ng, rows, zero_local=None, zero_border=None, twin_border=None):
    """Small integers, every sum exact, no damping anywhere.  Block b: rows 0 .. nb-1 of J_b are 2 I, so G_bb = 4 I and
    U_bb = 2 I; the same rows of C_b hold small even integers T_b (J_b'C_b = 2 T_b, W_b = T_b); the `rows` further rows of every
    block are zero in J_b and hold R = 2 I (B rows x ng, needs B rows >= ng) in the border, so S = R'R + sum T_b'T_b - W'W
    = 4 I exactly.  zero_local = (b, k): column k of J_b zero;  zero_border = j: border column j zero;  twin_border = (i, j),
    i < j: border column j a copy of column i (the pivot of j is 4 - 2^2).  Returns (J, y, damp)."""
    mb = nb + rows
    assert B * rows >= ng
    J = lsq.BorderedBlockDiagonal(B, mb, nb, ng)
    rng = np.random.default_rng(100 * nb + ng)
    damp = np.zeros(B * nb + ng)
    C = J.border
    for b in range(B):
        J.block(b)[:nb, :] = 2.0 * np.eye(nb)
        C[b * mb:b * mb + nb, :] = 2.0 * rng.integers(-2, 3, size=(nb, ng))
        for r in range(rows):
            j = b * rows + r
            if j < ng:
                C[b * mb + nb + r, j] = 2.0
    if zero_local is not None:
        b, k = zero_local
        J.block(b)[:, k] = 0.0
    if zero_border is not None:
        C[:, zero_border] = 0.0
    if twin_border is not None:
        i, j = twin_border
        C[:, j] = C[:, i]
    y = rng.integers(-3, 4, size=B * mb).astype(np.float64)
    return J, y, damp


# name: (B, nb, ng, rows, kwargs); the second line of cases sends S to the blocked factorisation (ng >= 32)
FAILURES = {
    "local": (3, 2, 3, 1, dict(zero_local=(1, 1))),
    "border": (3, 2, 3, 1, dict(zero_border=1)),
    "twin": (3, 2, 3, 1, dict(twin_border=(0, 2))),
    "both": (3, 2, 3, 1, dict(zero_local=(2, 0), zero_border=0)),
    "border blocked": (3, 17, 40, 14, dict(zero_border=37)),
    "twin blocked": (3, 5, 70, 24, dict(twin_border=(3, 66))),
    "both blocked": (3, 17, 40, 14, dict(zero_local=(1, 16), twin_border=(1, 2))),
}


def failure_case(name):
    B, nb, ng, rows, kw = FAILURES[name]
    return exact_operand(B, nb, ng, rows, **kw)


# ------------------------------------------------------------------------------------------ the global tanh fit
class TanhFit:
    """residual(b, i) = tanh(P[i] . a_b + Q[b, i] . s) - data(b, i): nb local weights a_b per data set, ng weights s shared by all.
    x = (a_0 .. a_{B-1}, s).  P (mb x nb) and Q (B mb x ng) are fixed features; the data come from known weights plus noise."""

    def __init__(self, B, mb, nb, ng, seed=42):
        self.shape = (B, mb, nb, ng)
        rng = np.random.default_rng(seed)
        self.P = rng.standard_normal((mb, nb)) / np.sqrt(nb)
        self.Q = rng.standard_normal((B * mb, ng)) / np.sqrt(ng)
        self.m, self.n = B * mb, B * nb + ng
        truth = np.concatenate([0.5 * rng.standard_normal(B * nb), 0.5 * rng.standard_normal(ng)])
        self.data = np.tanh(self.arg(truth)) + 1e-3 * rng.standard_normal(self.m)
        self.x0 = np.zeros(self.n)

    def arg(self, x):
        B, mb, nb, ng = self.shape
        loc = x[:B * nb].reshape((B, nb))
        return (loc @ self.P.T).reshape(-1) + self.Q @ x[B * nb:]

    def f_(self, out, x):
        out[:] = np.tanh(self.arg(x)) - self.data

    def fill(self, J, x):                         # J: a BorderedBlockDiagonal (views into J.data)
        B, mb, nb, ng = self.shape
        d = 1.0 - np.tanh(self.arg(x)) ** 2
        for b in range(B):
            J.block(b)[:, :] = d[b * mb:(b + 1) * mb, None] * self.P
        J.border[:, :] = d[:, None] * self.Q

    def fill_dense(self, Jm, x):                  # Jm: the dense m x n matrix of the same problem
        B, mb, nb, ng = self.shape
        T = lsq.BorderedBlockDiagonal(B, mb, nb, ng)
        self.fill(T, x)
        Jm[:, :] = T.toarray()

    def bordered_problem(self, g=True, x0=None):
        B, mb, nb, ng = self.shape
        return lsq.LeastSquaresProblem(x=(self.x0 if x0 is None else x0).copy(), y=np.zeros(self.m), f_=self.f_,
                                       g_=self.fill if g else None, J=lsq.BorderedBlockDiagonal(B, mb, nb, ng))

    def dense_problem(self, x0=None):
        return lsq.LeastSquaresProblem(x=(self.x0 if x0 is None else x0).copy(), y=np.zeros(self.m), f_=self.f_,
                                       g_=self.fill_dense, J=np.zeros((self.m, self.n), order="F"))


FITS = [(12, 20, 3, 70), (12, 20, 3, 8)]          # nb + ng > 64 and <= 64
