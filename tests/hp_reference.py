"""The accuracy tier's reference: the direct solves in numpy.longdouble (64-bit mantissa on x86-64, eps = 2^-63 = 1.08e-19:
three to four decimal digits beyond fp64), so that fp64 LAPACK's own error on an operand can be MEASURED and the device held
to a multiple of it (tests/accuracy_common.py, tests/test_h_gpu_accuracy.py, tests/test_i_gpu_accuracy_dense.py).

Plain numpy: vector operations per column / row, no Python loop over entries.  Inputs are fp64 arrays (converted exactly) or
longdouble arrays (taken as they are: a column-scaled operand V diag(s) is formed in longdouble by the caller and passed in).
Every result is longdouble.

    normal_solve(A, y, damp)       (A'A + diag(damp)) x = A'y by an unblocked Cholesky and two triangular solves
    arrowhead_solve(J, y, damp)    the same equations for a BorderedBlockDiagonal: eliminate per block, Schur complement,
                                   back-substitute (the algebra of block_solve in tests/test_f_gpu_bordered.py)
    inv_gram(A)                    inv(A'A) from the Cholesky factor; for a BorderedBlockDiagonal the B local diagonal blocks
                                   and the shared block of inv(J'J)
    lstsq_qr(A, y)                 min ||A x - y|| by Householder QR (no pivoting: full column rank is the caller's promise);
                                   y may be a matrix of right-hand sides: one factorisation, one solution per column
    minnorm_solve(W, c)            the minimum-norm z with W z = c, W of full ROW rank: Householder QR of W'
    minnorm_from_factors(B, W, y)  A^+ y = W^+ B^+ y for A = B W given by two full-rank factors (rank-deficient A, exact rank:
                                   tests/rankdef_common.py); minnorm_gram_solve: the same W^+ by the Cholesky factor of W W'
    pivoted_truncated_solve(A, y, jpvt, r)
                                   the xGELSY solution in longdouble for GIVEN pivots and rank: r Householder steps on A[:, jpvt],
                                   then the minimum-norm solution of [R11 R12] z = (Q'y)(1:r)
    normal_solve_refined(A, y, G), minnorm_gram_refined(W, c, G)
                                   the two solves above from a Gram matrix that the caller formed EXACTLY, plus one step of
                                   refinement: the affordable form for operands with hundreds of columns
"""
import numpy as np

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)          # 2^-63 where long double is the x87 format


def ld(a):
    return np.asarray(a).astype(LD)


def cholesky_upper(G):
    """U upper triangular with U'U = G (the upper triangle of G is read).  Left-looking, one row of U per step."""
    G = ld(G)
    n = G.shape[0]
    U = np.zeros((n, n), dtype=LD)
    for j in range(n):
        v = G[j, j:] - U[:j, j] @ U[:j, j:]
        if not v[0] > 0:
            raise np.linalg.LinAlgError("longdouble Cholesky: pivot %d is not positive" % j)
        U[j, j:] = v / np.sqrt(v[0])
    return U


def solve_upper(U, b):
    """x with U x = b; b a vector or a matrix of right-hand sides."""
    x = ld(b).copy()
    for i in range(U.shape[0] - 1, -1, -1):
        x[i] = (x[i] - U[i, i + 1:] @ x[i + 1:]) / U[i, i]
    return x


def solve_upper_t(U, b):
    """x with U'x = b."""
    x = ld(b).copy()
    for i in range(U.shape[0]):
        x[i] = (x[i] - U[:i, i] @ x[:i]) / U[i, i]
    return x


def chol_solve(U, b):
    return solve_upper(U, solve_upper_t(U, b))


def gram(A, damp=None):
    A = ld(A)
    G = A.T @ A
    if damp is not None:
        G = G + np.diag(ld(damp))
    return G


def normal_solve(A, y, damp=None):
    A = ld(A)
    return chol_solve(cholesky_upper(gram(A, damp)), A.T @ ld(y))


def _inv_from_factor(U):
    Ui = solve_upper(U, np.eye(U.shape[0], dtype=LD))          # inv(U), upper triangular
    return Ui @ Ui.T


def _is_bordered(J):
    return hasattr(J, "border_block")


def arrowhead_parts(J, damp=None, colscale=None):
    """Per block (G_b, E_b, A_b, C_b) and the shared S0 = C'C (+ damping) of a BorderedBlockDiagonal, in longdouble.
    colscale: n factors s (the effective Jacobian is J diag(s), formed here without rounding to fp64)."""
    B, nb, ng = J.nblocks, J.nb, J.ng
    s = None if colscale is None else ld(colscale)
    d = None if damp is None else ld(damp)
    blocks = []
    S0 = np.zeros((ng, ng), dtype=LD)
    for b in range(B):
        A, Cb = ld(J.block(b)), ld(J.border_block(b))
        if s is not None:
            A, Cb = A * s[b * nb:(b + 1) * nb], Cb * s[B * nb:]
        G = A.T @ A
        if d is not None:
            G = G + np.diag(d[b * nb:(b + 1) * nb])
        blocks.append((G, A.T @ Cb, A, Cb))
        S0 = S0 + Cb.T @ Cb
    if d is not None:
        S0 = S0 + np.diag(d[B * nb:])
    return blocks, S0


def arrowhead_solve(J, y, damp=None, colscale=None):
    B, mb, nb, ng = J.nblocks, J.mb, J.nb, J.ng
    y = ld(y)
    blocks, S = arrowhead_parts(J, damp, colscale)
    rg = np.zeros(ng, dtype=LD)
    keep = []
    for b, (G, E, A, Cb) in enumerate(blocks):
        yb = y[b * mb:(b + 1) * mb]
        W = chol_solve(cholesky_upper(G), np.column_stack([E, A.T @ yb]))      # inv(G) [A'C_b, A'y_b]
        S = S - E.T @ W[:, :ng]
        rg = rg + Cb.T @ yb - E.T @ W[:, ng]
        keep.append(W)
    xg = chol_solve(cholesky_upper(S), rg)
    return np.concatenate([W[:, ng] - W[:, :ng] @ xg for W in keep] + [xg])


def inv_gram(A, colscale=None):
    """inv(A'A) of a dense block; for a BorderedBlockDiagonal: ([local diagonal block b of inv(J'J)], the shared block):
    with W_b = inv(G_b) E_b and S the Schur complement, shared = inv(S) and local_b = inv(G_b) + W_b inv(S) W_b'."""
    if not _is_bordered(A):
        return _inv_from_factor(cholesky_upper(gram(A)))
    blocks, S = arrowhead_parts(A, None, colscale)
    Gi, Ws = [], []
    for G, E, _, _ in blocks:
        U = cholesky_upper(G)
        W = chol_solve(U, E)
        S = S - E.T @ W
        Gi.append(_inv_from_factor(U))
        Ws.append(W)
    Si = _inv_from_factor(cholesky_upper(S))
    return [Gi[b] + Ws[b] @ Si @ Ws[b].T for b in range(len(blocks))], Si


def lstsq_qr(A, y):
    """Householder QR applied to [A | y], then one back substitution.  y: a vector, or an m x r matrix of right-hand sides
    (the result is then n x r; every column carries the bits of its own single solve: a reflector is applied column by column).
    The work array is [A | y] transposed, so that a reflector runs over contiguous memory (tall operands: half the time)."""
    A = ld(A)
    m, n = A.shape
    RT = np.ascontiguousarray(np.column_stack([A, ld(y)]).T)
    for j in range(n):
        v = RT[j, j:].copy()
        alpha = np.sqrt(v @ v)
        if alpha == 0:
            raise np.linalg.LinAlgError("longdouble QR: column %d is zero" % j)
        v[0] += alpha if v[0] >= 0 else -alpha
        v = v / np.sqrt(v @ v)
        RT[j:, j:] -= 2 * np.outer(RT[j:, j:] @ v, v)
    R = RT.T
    return solve_upper(np.triu(R[:n, :n]), R[:n, n] if np.ndim(y) == 1 else R[:n, n:])


def _reflect(RT, steps):
    """The first `steps` Householder reflectors of the QR of RT' (RT holds the columns as its rows, as in lstsq_qr), applied in
    place; returns their unit vectors v_j (H_j = I - 2 v_j v_j' on the entries j..)."""
    vs = []
    for j in range(steps):
        v = RT[j, j:].copy()
        alpha = np.sqrt(v @ v)
        if alpha == 0:
            raise np.linalg.LinAlgError("longdouble QR: column %d is zero" % j)
        v[0] += alpha if v[0] >= 0 else -alpha
        v = v / np.sqrt(v @ v)
        RT[j:, j:] -= 2 * np.outer(RT[j:, j:] @ v, v)
        vs.append(v)
    return vs


def minnorm_solve(W, c):
    """The minimum-norm z with W z = c for W (r x n, full row rank: the caller's promise): W' = Q [R; 0] by Householder, then
    z = Q [R'^-1 c; 0].  Backward stable: cond(W) enters once (the Cholesky factor of W W' would square it)."""
    RT = np.ascontiguousarray(ld(W))            # the rows of W are the columns of W'
    r, n = RT.shape
    vs = _reflect(RT, r)
    R = np.triu(RT[:, :r].T)
    z = np.zeros(n, dtype=LD)
    z[:r] = solve_upper_t(R, ld(c))
    for j in range(r - 1, -1, -1):
        z[j:] -= 2 * vs[j] * (vs[j] @ z[j:])
    return z


def minnorm_gram_solve(W, c):
    """The same z = W'(W W')^-1 c by the longdouble Cholesky factor of W W' (cond(W)^2: for well-conditioned W only)."""
    W = ld(W)
    return W.T @ chol_solve(cholesky_upper(W @ W.T), ld(c))


def minnorm_from_factors(B, W, y, z=None):
    """A^+ y for A = B W, B (m x r) of full column rank and W (r x n) of full row rank: A^+ = W^+ B^+, so z = B^+ y by lstsq_qr
    (pass it in to reuse it for another W) and x = W^+ z by minnorm_solve.  No rank decision, no pivoting: the reference does
    not depend on the algorithm under test."""
    if z is None:
        z = lstsq_qr(B, y)
    return minnorm_solve(W, z)


def pivoted_truncated_solve(A, y, jpvt, r):
    """xGELSY's answer for pivots jpvt and rank r, in longdouble: r Householder steps on [A[:, jpvt] | y], the minimum-norm
    solution of [R11 R12] z = (Q'y)(1:r), x[jpvt] = z."""
    A = ld(A)
    n = A.shape[1]
    jpvt = np.asarray(jpvt)
    x = np.zeros(n, dtype=LD)
    if r == 0:
        return x
    RT = np.ascontiguousarray(np.column_stack([A[:, jpvt], ld(y)]).T)
    _reflect(RT, r)
    x[jpvt] = minnorm_solve(np.triu(RT[:n, :r].T), RT[n, :r])
    return x


def normal_solve_refined(A, y, G, damp=None):
    """(A'A + diag(damp)) x = A'y with the Gram matrix G = A'A GIVEN -- exact where the caller can form it exactly (integer
    factors) -- by its Cholesky factor and one step of refinement on the residual A'(y - A x) - damp x, formed in longdouble
    without G.  For the large operands of tests/rankdef_common.py, where n Householder steps in longdouble take a quarter of a
    minute: the Cholesky factor costs n^3 / 3, and the refinement step takes the error from cond(G) 2^-64 to its square."""
    A, y, G = ld(A), ld(y), ld(G)
    d = np.zeros(A.shape[1], dtype=LD) if damp is None else ld(damp)
    U = cholesky_upper(G + np.diag(d))
    x = chol_solve(U, A.T @ y)
    return x + chol_solve(U, A.T @ (y - A @ x) - d * x)


def minnorm_gram_refined(W, c, G):
    """The minimum-norm z = W'u, (W W') u = c with G = W W' GIVEN (exact for an integer W), one step of refinement on
    c - W (W'u)."""
    W, c = ld(W), ld(c)
    U = cholesky_upper(G)
    u = chol_solve(U, c)
    u = u + chol_solve(U, c - W @ (W.T @ u))
    return W.T @ u
