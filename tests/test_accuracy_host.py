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
   every block."""
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
