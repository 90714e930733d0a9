"""Accuracy tier, host part (no device): the longdouble reference (tests/hp_reference.py) and the acceptance rule
(tests/accuracy_common.py) are checked here before tests/test_h_gpu_accuracy.py relies on them.

1. On every shape family of the device tier the longdouble solutions satisfy their own equations to
   8 n 2^-63 (||G||_F ||x|| + ||r||): a first-order backward-error bound of a Cholesky / Householder solve with unit
   roundoff 2^-64, with the slack n for the length-n (Gram: length-m, but m eps stays below it here) accumulations.
2. Against mpmath at 40 digits on two tiny operands (12 x 5, cond(A'A) = 1e6): the forward error of a backward-stable solve
   is at most c n u cond; 8 n 2^-63 cond = 4e-12 is taken, two orders below what fp64 LAPACK can reach there.
3. The rule separates right from subtly wrong: an fp64 numpy stand-in of the device algorithm (Gram matrix in 32-row chunks
   split four ways, right-looking Cholesky multiplying by a reciprocal square root) passes it on every operand family, and the
   same stand-in with its reciprocal square root rounded through float32 and not corrected fails it on every family -- in
   every block.
4. The dense tier (tests/test_i_gpu_accuracy_dense.py): several right-hand sides in one longdouble factorisation carry the bits
   of single solves; far operands have plain's solution bit for bit; the reference's residuals on the new operands; a second
   fp64 Householder QR (rows permuted) passes the rule on EVERY operand of the device tier; the fp64 normal equations do not.
5. The product bound (tests/test_i_gpu_accuracy_products.py) accepts any summation order and rejects a float32 x and one
   dropped entry of the smallest row."""
import numpy as np
import pytest

import accuracy_common as ac
import hp_reference as hp

LD = hp.LD
NBS = list(ac.BD_NBS)
BB_SHAPES = [(5, 3), (15, 1), (16, 17), (40, 24), (1, 63), (63, 1), (3, 2), (16, 1), (20, 12)]


def nrm(v):
    v = hp.ld(v).reshape(-1)
    return np.sqrt(v @ v)


def test_longdouble_is_the_x87_format():
    assert np.finfo(LD).nmant >= 63 and hp.EPS_LD <= 1.1e-19


def residual_ok(G, x, r, n):
    return nrm(G @ x - r) <= 8 * n * LD(2.0) ** -63 * (nrm(G) * nrm(x) + nrm(r))


# ------------------------------------------------------------------------------------------ 1. the reference's own residuals
@pytest.mark.parametrize("family", ac.FAMILIES)
@pytest.mark.parametrize("nb", NBS)
def test_normal_solve_residual_block_shapes(family, nb):
    op = ac.bd_operand(family, 2, 70, nb, 40 + nb)
    for b in range(2):
        A, yb = hp.ld(op.J.block(b)), hp.ld(op.y[b * 70:(b + 1) * 70])
        for damp in (op.damp[b * nb:(b + 1) * nb], None):
            x = hp.normal_solve(A, yb, damp)
            assert x.dtype == LD
            assert residual_ok(hp.gram(A, damp), x, A.T @ yb, nb), (family, nb, b, damp is None)
        if family in ("plain", "graded", "ill"):
            G = hp.gram(A)
            Ci = hp.inv_gram(A)
            assert nrm(G @ Ci - np.eye(nb)) <= 8 * nb * LD(2.0) ** -63 * (nrm(G) * nrm(Ci) + np.sqrt(LD(nb)))


@pytest.mark.parametrize("family", ["plain", "graded", "ill"])
@pytest.mark.parametrize("n", [9, 70, 129, 200])
def test_normal_solve_residual_dense_shapes(family, n):
    op = ac.dense_operand(family, 3 * n + 5, n, 60 + n)
    A, y = hp.ld(op.J), hp.ld(op.y)
    x = hp.normal_solve(A, y, op.damp)
    assert residual_ok(hp.gram(A, op.damp), x, A.T @ y, n)


def arrowhead_residual(J, y, damp, x):
    """||G x - r||, ||G||_F and ||r|| of the arrowhead normal equations, block by block in longdouble."""
    B, mb, nb, ng = J.nblocks, J.mb, J.nb, J.ng
    blocks, S0 = hp.arrowhead_parts(J, damp)
    y = hp.ld(y)
    xg = x[B * nb:]
    res2, r2, g2 = LD(0), LD(0), np.sum(S0 * S0)
    sh, rg = S0 @ xg, np.zeros(ng, dtype=LD)
    for b, (G, E, A, Cb) in enumerate(blocks):
        xb, yb = x[b * nb:(b + 1) * nb], y[b * mb:(b + 1) * mb]
        rb = A.T @ yb
        d = G @ xb + E @ xg - rb
        res2 += d @ d
        r2 += rb @ rb
        g2 += np.sum(G * G) + 2 * np.sum(E * E)
        sh = sh + E.T @ xb
        rg = rg + Cb.T @ yb
    res2 += (sh - rg) @ (sh - rg)
    return np.sqrt(res2), np.sqrt(g2), np.sqrt(r2 + rg @ rg)


@pytest.mark.parametrize("family", ac.FAMILIES)
@pytest.mark.parametrize("nb,ng", BB_SHAPES)
def test_arrowhead_solve_residual(family, nb, ng):
    B, mb = 5, 96
    op = ac.bb_operand(family, B, mb, nb, ng, 7 + nb + ng)
    n = B * nb + ng
    x = hp.arrowhead_solve(op.J, op.y, op.damp)
    res, gn, rn = arrowhead_residual(op.J, op.y, op.damp, x)
    assert res <= 8 * n * LD(2.0) ** -63 * (gn * nrm(x) + rn), (family, nb, ng)
    if family in ("plain", "graded", "ill"):
        # the block form of inv(J'J) against the dense longdouble inverse of the same matrix, in the covariance metric: both are
        # backward-stable inverses, so they differ by at most c n u cond(G) with G column-equilibrated (the metric's scaling)
        loc, shared = hp.inv_gram(op.J)
        D = op.J.toarray()
        full = hp.inv_gram(D)
        sd = np.sqrt(np.diag(full))
        tol = 8 * n * LD(2.0) ** -63 * float(np.linalg.cond(D / ac.colnorms(D).astype(float)) ** 2)
        for b in range(B):
            sl = slice(b * nb, (b + 1) * nb)
            assert np.max(np.abs(loc[b] - full[sl, sl]) / np.outer(sd[sl], sd[sl])) <= tol, (family, nb, ng, b)
        sl = slice(B * nb, n)
        assert np.max(np.abs(shared - full[sl, sl]) / np.outer(sd[sl], sd[sl])) <= tol


def test_arrowhead_solve_column_scaled_is_the_scaled_operand():
    op = ac.bb_operand("graded", 5, 96, 16, 17, 3)
    x1 = hp.arrowhead_solve(op.V, op.y, op.damp, colscale=op.s)
    x2 = hp.arrowhead_solve(op.J, op.y, op.damp)               # fl(V diag(s)): one fp64 rounding per entry apart
    S = np.concatenate(ac.bb_colnorms(op)[0] + [ac.bb_colnorms(op)[1]])
    assert 0 < ac.solve_err(x2, x1, S) <= 64 * 2.0 ** -53


@pytest.mark.parametrize("c", [1, 5, 7, 7.75])
def test_lstsq_qr_normal_equations(c):
    rng = np.random.default_rng(int(100 * c))
    A = ac.ill_matrix(rng, 640, 64, decades=c)
    y = rng.standard_normal(640)
    x = hp.lstsq_qr(A, y)
    Al, yl = hp.ld(A), hp.ld(y)
    # A'(A x - y) = 0 up to the backward error E of the factorisation: ||A'E x|| + ||E'r|| <= 8 n u ||A||_F (||A||_F ||x|| + ||y||)
    assert nrm(Al.T @ (Al @ x - yl)) <= 8 * 64 * LD(2.0) ** -63 * nrm(Al) * (nrm(Al) * nrm(x) + nrm(yl))


@pytest.mark.parametrize("mb,nb", [(40, 17), (257, 64)])
def test_lstsq_qr_graded_and_stacked_damped(mb, nb):
    rng = np.random.default_rng(mb)
    A = rng.standard_normal((mb, nb)) / np.sqrt(mb) * ac.grading(nb, 6.0)
    y = rng.standard_normal(mb)
    damp = 0.1 * np.sum(A * A, axis=0)
    for M, rhs in ((hp.ld(A), hp.ld(y)),
                   (np.vstack([hp.ld(A), np.diag(np.sqrt(hp.ld(damp)))]), np.concatenate([hp.ld(y), np.zeros(nb, dtype=LD)]))):
        # column-equilibrated: the normal-equation residual is judged in the scaling the QR solve is invariant under
        S = ac.colnorms(M)
        Ms = M / S
        x = hp.lstsq_qr(M, rhs)
        assert nrm(Ms.T @ (Ms @ (S * x) - rhs)) <= 8 * nb * LD(2.0) ** -63 * nrm(Ms) * (nrm(Ms) * nrm(S * x) + nrm(rhs))
    # the damped stacked least-squares problem IS the damped normal equations
    xs = hp.lstsq_qr(np.vstack([hp.ld(A), np.diag(np.sqrt(hp.ld(damp)))]), np.concatenate([hp.ld(y), np.zeros(nb, dtype=LD)]))
    S = ac.colnorms(A)
    assert ac.solve_err(xs, hp.normal_solve(A, y, damp), S) <= 1e-15


# ------------------------------------------------------------------------------------------ 2. against mpmath
def test_against_mpmath_on_two_tiny_operands():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        A = ac.ill_matrix(rng, 12, 5)                           # cond(A'A) = 1e6
        y = rng.standard_normal(12)
        damp = 1e-9 * np.sum(A * A, axis=0)
        Am = mp.matrix(A.tolist())
        ym = mp.matrix(y.tolist())
        tol = 8 * 5 * 2.0 ** -63 * 1e6

        def close(x, xm):
            xm = np.array([mp.mpf(v) for v in xm], dtype=object).reshape(np.shape(x))
            num = mp.sqrt(sum((mp.mpf(float(a)) + mp.mpf(float(a - LD(float(a)))) - b) ** 2 for a, b in zip(np.ravel(x), np.ravel(xm))))
            return num / mp.sqrt(sum(b ** 2 for b in np.ravel(xm)))

        G = Am.T * Am
        xm = mp.lu_solve(G, Am.T * ym)
        assert close(hp.normal_solve(A, y), xm) <= tol
        assert close(hp.lstsq_qr(A, y), xm) <= tol
        Gd = G + mp.diag([mp.mpf(float(d)) for d in damp])
        assert close(hp.normal_solve(A, y, damp), mp.lu_solve(Gd, Am.T * ym)) <= tol
        assert close(hp.inv_gram(A), G ** -1) <= tol
        # ... and fp64 LAPACK is further from it than the longdouble reference, by orders: there is something to measure
        e64 = close(hp.ld(np.linalg.solve(A.T @ A, A.T @ y)), xm)
        assert e64 > 100 * close(hp.normal_solve(A, y), xm)


# ------------------------------------------------------------------------------------------ 3. the rule separates
def standin_pieces(op, nb, degraded, damp):
    J = op.J
    out = []
    for b in range(J.nblocks):
        A, yb = J.block(b), op.y[b * J.mb:(b + 1) * J.mb]
        db = None if damp is None else damp[b * nb:(b + 1) * nb]
        x = ac.standin_solve(A, yb, db, degraded)
        x_hp = hp.normal_solve(A, yb, db)
        G = A.T @ A if db is None else A.T @ A + np.diag(db)
        S = ac.colnorms(A)
        out.append(("block %d" % b, ac.solve_err(x, x_hp, S), ac.solve_err(np.linalg.solve(G, A.T @ yb), x_hp, S), nb))
    return out


@pytest.mark.parametrize("family", ac.FAMILIES)
@pytest.mark.parametrize("nb", NBS)
def test_rule_on_the_solve_standin_passes_and_degraded_fails(family, nb):
    op = ac.bd_operand(family, ac.BD_B, ac.BD_MB, nb, ac.bd_seed(nb))         # the device tier's own operands
    for damp in ((op.damp, None) if family == "ill" else (op.damp,)):
        good = standin_pieces(op, nb, False, damp)
        ac.judge("stand-in %s nb=%d %s" % (family, nb, "damped" if damp is not None else "undamped"), good)
        bad = standin_pieces(op, nb, True, damp)
        print("   degraded: e_dev %s" % " ".join("%.2e" % p[1] for p in bad))
        assert not any(ac.accepted(d, r, k) for _, d, r, k in bad), (family, nb, bad)
        with pytest.raises(AssertionError):
            ac.judge("degraded", bad)


@pytest.mark.parametrize("family", ["plain", "graded", "ill"])
@pytest.mark.parametrize("nb", NBS)
def test_rule_on_the_covariance_standin_passes_and_degraded_fails(family, nb):
    op = ac.bd_operand(family, ac.BD_B, ac.BD_MB, nb, ac.bd_seed(nb))
    rng = np.random.default_rng(nb)
    for b in range(ac.BD_B):
        A = op.J.block(b)
        f = rng.standard_normal(70)
        H = hp.inv_gram(A) * ac.s2_of(f, 70 - nb)
        s2 = np.sum(f ** 2) / (70 - nb)
        Cref = s2 * np.linalg.inv(A.T @ A)
        good = s2 * ac.standin_inv(A)
        ac.judge("stand-in covariance %s nb=%d block %d" % (family, nb, b), ac.cov_pieces("block", good, np.sqrt(np.diag(good)), Cref, H, nb))
        bad = s2 * ac.standin_inv(A, degraded=True)
        pieces = ac.cov_pieces("block", bad, np.sqrt(np.diag(bad)), Cref, H, nb)
        assert not any(ac.accepted(d, r, k) for _, d, r, k in pieces), (family, nb, b, pieces)


def test_rule_floor_and_factor():
    assert ac.bound(0.0, 5) == 16 * 16 * 2.0 ** -53            # the floor: LAPACK happened to be exact
    assert ac.bound(0.0, 64) == 16 * 64 * 2.0 ** -53
    assert ac.bound(1e-10, 64) == 16e-10
    assert not ac.accepted(np.nan, 1.0, 5) and not ac.accepted(np.inf, 1.0, 5)


def test_rule_floor_is_capped_at_64_unknowns():
    """Unchanged for every piece of the block solvers (k <= 64); a 321-column norm gets the floor of 64, not of 321."""
    for k in (1, 5, 16, 17, 33, 48, 63, 64):
        assert ac.bound(0.0, k) == 16 * max(16, k) * 2.0 ** -53
        assert ac.bound(3e-13, k) == 16 * 3e-13
    for k in (65, 70, 129, 200, 321, 384):
        assert ac.bound(0.0, k) == 16 * 64 * 2.0 ** -53
    assert ac.accepted(16 * 64 * 2.0 ** -53, 0.0, 321) and not ac.accepted(16 * 65 * 2.0 ** -53, 0.0, 321)


# ------------------------------------------------------------------------------------------ 4. the dense tier's reference and rule
def test_lstsq_qr_multi_rhs_has_the_bits_of_single_solves():
    for m, n, family in ((700, 130, "graded"), (97, 31, "ill")):
        ref = ac.qr_ref(family, m, n)
        for A, Y in ((hp.ld(ref.A), hp.ld(ref.Y)), ac.stacked(hp.ld(ref.A), hp.ld(ref.Y), ref.damp)):
            X = hp.lstsq_qr(A, Y)
            assert X.shape == (n, 2) and X.dtype == LD
            for c in range(2):
                assert np.array_equal(X[:, c], hp.lstsq_qr(A, Y[:, c]))


def test_far_operand_has_the_bits_of_plain():
    """Operand and y times 2^+-100, damping times 2^+-200: the longdouble solution is plain's bit for bit (what QrRef relies on),
    and the fp64 operand itself is plain's scaled exactly."""
    m, n = 300, 20
    plain = ac.qr_ref("plain", m, n)
    for family, f in (("far+", 2.0 ** 100), ("far-", 2.0 ** -100)):
        far = ac.QrRef(family, m, n)
        assert np.array_equal(far.A, plain.A * f) and np.array_equal(far.Y, plain.Y * f) and np.array_equal(far.damp, plain.damp * f * f)
        assert np.array_equal(hp.lstsq_qr(far.A, far.Y), plain.x_hp(None, False))
        assert np.array_equal(hp.lstsq_qr(*ac.stacked(hp.ld(far.A), hp.ld(far.Y), far.damp)), plain.x_hp(None, True))
        assert np.array_equal(far.S, plain.S * LD(f))


@pytest.mark.parametrize("m,n,family", [(700, 130, "plain"), (700, 130, "graded"), (700, 130, "ill"), (33000, 8, "plain"),
                                        (33000, 8, "graded")])
def test_lstsq_qr_residual_on_the_dense_tier_operands(m, n, family):
    """A'(A x - y) = 0 to longdouble level for both right-hand sides, undamped and stacked, column-equilibrated (the scaling a QR
    solve is invariant under): the bound of test_lstsq_qr_graded_and_stacked_damped."""
    ref = ac.qr_ref(family, m, n)
    for damped in (False, True):
        A, Y = hp.ld(ref.A), hp.ld(ref.Y)
        if damped:
            A, Y = ac.stacked(A, Y, ref.damp)
        S = ac.colnorms(A)
        As = A / S
        for c, rhs in enumerate(ac.RHS):
            x = ref.x_hp(rhs, damped)
            assert nrm(As.T @ (As @ (S * x) - Y[:, c])) <= 8 * n * LD(2.0) ** -63 * nrm(As) * (nrm(As) * nrm(S * x) + nrm(Y[:, c])), (rhs, damped)


def permuted_qr_solve(A, y, seed):
    """fp64 Householder QR of the row-permuted problem: the same solution, another realisation of LAPACK's rounding errors."""
    p = np.random.default_rng(seed).permutation(A.shape[0])
    return ac.qr_fp64_solve(A[p], y[p])


QR_OPERANDS = ([(m, n, f) for (m, n) in ac.QR_PANEL_SHAPES for f in ac.QR_PANEL_FAMILIES] +
               [(m, ac.QR_ROW_VARIANT_N, f) for m in ac.QR_ROW_VARIANT_MS for f in ("graded", "ill")] +
               [(m, n, f) for (m, n) in ac.QR_TSQR_SHAPES for f in ac.QR_TSQR_FAMILIES])


@pytest.mark.parametrize("m,n,family", QR_OPERANDS)
def test_rule_accepts_another_householder_qr_on_every_dense_operand(m, n, family):
    """The 'reference alone' condition of the QR groups of tests/test_i_gpu_accuracy_dense.py: on every operand, right-hand side
    and damping of the device tier a second fp64 Householder QR (rows permuted) passes the rule that the device must pass."""
    ref = ac.qr_ref(family, m, n)
    pieces = []
    for damped in (False, True):
        for rhs in ac.RHS:
            x = permuted_qr_solve(*ref.problem(rhs, damped), seed=m + n)
            pieces.append(("%s %s" % (rhs, "damped" if damped else "undamped"), ref.err(x, rhs, damped), ref.e_ref(rhs, damped), n))
    ac.judge("permuted QR %dx%d %s" % (m, n, family), pieces)


def normal_equations_solve(A, y):
    return np.linalg.solve(A.T @ A, A.T @ y)


@pytest.mark.parametrize("m,n", [(700, 130), (1000, 321)])
def test_rule_rejects_the_normal_equations_and_the_consistent_rhs_is_the_sharper_one(m, n):
    """ill (cond 1e3), undamped: a backward-stable QR has an error of cond u, the fp64 normal equations cond^2 u, and the rule
    must tell them apart.  Consistent y (residual at rounding level): 1.5e-11 against a bound of 3.7e-13 at 700 x 130 (41 x
    beyond), 2.3e-11 against 6.5e-13 at 1000 x 321 (36 x).  Random y: the residual term cond^2 u ||r|| / (||A|| ||x||) enters the
    QR's own error as well, e_ref doubles (4.8e-14 against 2.3e-14; 6.3e-14 against 4.1e-14) and the margin halves (19 x, 20 x).
    The expectation that the random y hides the normal equations altogether did NOT hold on these operands (||x|| ~ 1 / sigma_min
    keeps the residual term small); what holds, and is asserted, is that the consistent y gives the tighter bound -- which is
    why the device tier runs both."""
    ref = ac.qr_ref("ill", m, n)
    e_ref = {}
    for rhs in ac.RHS:
        e = ref.err(normal_equations_solve(*ref.problem(rhs, False)), rhs, False)
        e_ref[rhs] = ref.e_ref(rhs, False)
        print("normal equations, %s y: e %.3e, e_ref %.3e, bound %.3e" % (rhs, e, e_ref[rhs], ac.bound(e_ref[rhs], n)))
        assert not ac.accepted(e, e_ref[rhs], n)
    assert e_ref["consistent"] < e_ref["random"]


# ------------------------------------------------------------------------------------------ 5. the product bound
def product_case():
    S = ac.ragged_pattern(500, 40, 0.5, 540)
    r, c = ac.product_scales(500, 40, 580)
    (x, y), _ = ac.product_vectors(r, c, 7)
    return S.toarray() * r[:, None] * c, x, y


def pairwise(t):
    while t.shape[1] > 1:
        if t.shape[1] % 2:
            t = np.column_stack([t, np.zeros(t.shape[0])])
        t = t[:, 0::2] + t[:, 1::2]
    return t[:, 0]


def test_product_bound_accepts_any_summation_order():
    A, x, y = product_case()
    K = np.count_nonzero(A, axis=1)
    ref, mag = ac.product_reference(A, x, 1.5, -0.5, y)
    assert K[3] == 0 and K[5] == 39 and mag.min() > 0 and float(mag.max() / mag.min()) > 1e10
    T = A * x                                   # the rounded terms a_ik x_k
    fwd = np.zeros(500)
    for k in range(40):
        fwd = fwd + T[:, k]
    rev = np.zeros(500)
    for k in range(39, -1, -1):
        rev = rev + T[:, k]
    for name, dot in (("numpy", A @ x), ("forward", fwd), ("reversed", rev), ("pairwise", pairwise(T))):
        ac.judge_product("host " + name, 1.5 * dot + -0.5 * y, ref, K, 3, mag)


def test_product_bound_rejects_a_float32_x_and_a_dropped_entry():
    A, x, y = product_case()
    K = np.count_nonzero(A, axis=1)
    ref, mag = ac.product_reference(A, x, 1.5, -0.5, y)
    q, _ = ac.product_excess(1.5 * (A @ x.astype(np.float32).astype(np.float64)) - 0.5 * y, ref, K, 3, mag)
    assert q > 1e3                              # 2^-24 against gamma_43: five orders
    # one entry of the row with the smallest scale: invisible to a normwise check
    i = int(np.argmin(np.where(K > 1, np.max(np.abs(A), axis=1), np.inf)))
    B = A.copy()
    B[i, np.flatnonzero(A[i])[0]] = 0.0
    out = 1.5 * (B @ x) - 0.5 * y
    full = 1.5 * (A @ x) - 0.5 * y
    assert np.max(np.abs(out - full)) <= 1e-12 * np.max(np.abs(full))          # a whole-vector scale, as the shape tier has it, passes
    q, worst = ac.product_excess(out, ref, K, 3, mag)
    assert worst == i and q > 1e3
    with pytest.raises(AssertionError):
        ac.judge_product("dropped entry", out, ref, K, 3, mag)
