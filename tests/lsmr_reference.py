"""A recording twin of the reference's LSMR solve, ldiv!(x, J, y[, damp], ::LSMR), in plain numpy at a chosen precision
(numpy.float64 or numpy.longdouble).  Written from the algorithm (Fong & Saunders, LSMR, SISC 2011, as the reference restates
it in src/utils/lsmr.jl and wraps it in src/solver/iterative_lsmr.jl):

    P     = 1 / sqrt(colsumabs2(J) (+ damp)), 0 where that sum is 0;   damp <- sqrt(damp)
    A     = [J; diag(damp)] diag(P),  b = [y; 0],  x0 = 0
    tolerances  atol = 1e-6, btol = 0.5 (damped) / 1e-6 (undamped), conlim = 1e8, maxiter = max(rows(A), n)
    guards      u is normalised only if beta > 0, and then v is advanced and normalised only if alpha > 0;
                the norm of the stacked vector [u_y; u_x] is sqrt(norm(u_y)^2 + norm(u_x)^2)
    result      x <- P .* x

The twin keeps, per iteration, every quantity a stopping rule looks at and the iterate, and per solve (iter, istop).  With
`iters=K` it runs exactly K iterations with the rules switched off (K = 0: the start, x = 0): the high-precision iterate at
the iteration at which another implementation stopped.  `maxiter` overrides the reference's max(rows, n) (the row-sharded
loop of the package takes it as an argument); `wide_sums` accumulates every sum in longdouble (see _wide).

Stopping rules, first hit wins, in this order (istop):
    7  iter >= maxiter          6  1 + test3 <= 1           5  1 + test2 <= 1          4  1 + t1 <= 1
    3  test3 <= 1/conlim        2  test2 <= atol            1  test1 <= rtol
    0  the loop never ran: A'b == 0 (b == 0 included)
with test1 = normr/normb, test2 = normAr/(normA normr), test3 = 1/condA, t1 = test1/(1 + normA normx/normb),
rtol = btol + atol normA normx/normb.  The `1 + t <= 1` comparisons are made in the twin's own precision.
"""
import numpy as np

ATOL, BTOL, BTOL_DAMPED, CONLIM = 1e-6, 1e-6, 0.5, 1e8
RULE_ORDER = (7, 6, 5, 4, 3, 2, 1)


class Record:
    """One solve.  `its` is a list of dicts (alpha, beta, test1, test2, test3, t1, rtol, normr, normAr, normx, normA, condA,
    x, fired) -- `x` the iterate P .* x_k, `fired` the tuple of every rule that holds at that iteration (in RULE_ORDER)."""

    def __init__(self):
        self.its = []
        self.iter = 0
        self.istop = 0
        self.x = None
        self.P = None
        self.damp_after = None
        self.maxiter = 0
        self.alpha0 = self.beta0 = None

    @property
    def nmul(self):
        return 2 * self.iter


def _nrm(v):
    return np.sqrt(v @ v)


def _wide(f):
    """f(*arrays) with every sum accumulated in longdouble and rounded once to the arrays' precision: another association of
    the same sums (what a tree reduction or a fused multiply-add changes), used to show that an exact zero does not depend on
    the order of summation."""
    def g(*a):
        return np.asarray(f(*[np.asarray(t, dtype=np.longdouble) for t in a])).astype(a[0].dtype)
    return g


def rules_that_hold(q, it, maxiter, atol, ctol, one):
    """Every rule whose condition is true for the quantities q of iteration `it`, in the order they are tried."""
    with np.errstate(invalid="ignore"):
        cond = {7: it >= maxiter, 6: one + q["test3"] <= one, 5: one + q["test2"] <= one, 4: one + q["t1"] <= one,
                3: q["test3"] <= ctol, 2: q["test2"] <= atol, 1: q["test1"] <= q["rtol"]}
    return tuple(k for k in RULE_ORDER if bool(cond[k]))


def ldiv_lsmr(J, y, damp=None, dtype=np.float64, iters=None, wide_sums=False, maxiter=None):
    T = dtype
    matvec, nrm, sumsq_cols = (lambda A, t: A @ t), _nrm, (lambda A: np.sum(A * A, axis=0))
    if wide_sums:
        matvec, sumsq_cols = _wide(matvec), _wide(sumsq_cols)
        nrm = lambda v: np.sqrt(_wide(lambda t: t @ t)(v))  # noqa: E731
    if hasattr(J, "colsumabs2"):       # an operator with @, .T, .shape (tests/trust_region_reference.py: Band), already in T
        sumsq_cols = lambda A: A.colsumabs2()  # noqa: E731
    else:
        J = np.asarray(J, dtype=T)
    y = np.asarray(y, dtype=T)
    m, n = J.shape
    damped = damp is not None
    one, zero = T(1), T(0)
    rec = Record()
    s = sumsq_cols(J)
    if damped:
        dtd = np.asarray(damp, dtype=T)
        if np.any(dtd != 0):
            s = s + dtd
        dg = np.sqrt(dtd)
        rec.damp_after = dg
    with np.errstate(divide="ignore"):
        P = np.where(s > 0, one / np.sqrt(np.where(s > 0, s, one)), zero).astype(T)
    rec.P = P
    atol, ctol = T(ATOL), one / T(CONLIM)
    btol = T(BTOL_DAMPED) if damped else T(BTOL)
    if maxiter is None:
        maxiter = max(m + (n if damped else 0), n)
    rec.maxiter = maxiter

    def A_v(v, alpha, uy, ux):            # u <- A v - alpha u
        t = P * v
        return matvec(J, t) - alpha * uy, (t * dg - alpha * ux) if damped else ux

    def At_u(uy, ux, beta, v):            # v <- A'u - beta v
        t = matvec(J.T, uy)
        if damped:
            t = t + ux * dg
        return P * t - beta * v

    def norm_u(uy, ux):
        if not damped:
            return nrm(uy)
        a, b = nrm(uy), nrm(ux)
        return np.sqrt(a * a + b * b)

    x = np.zeros(n, dtype=T)
    uy, ux = y.copy(), np.zeros(n, dtype=T)
    beta = norm_u(uy, ux)
    if beta > 0:
        uy, ux = uy * (one / beta), ux * (one / beta)
    v = At_u(uy, ux, zero, np.zeros(n, dtype=T))
    alpha = nrm(v)
    if alpha > 0:
        v = v * (one / alpha)
    rec.alpha0, rec.beta0 = alpha, beta
    zetabar, alphabar, rho, rhobar, cbar, sbar = alpha * beta, alpha, one, one, one, zero
    h, hbar = v.copy(), np.zeros(n, dtype=T)
    betadd, betad, rhodold, tautildeold, thetatilde, zeta, d = beta, zero, one, zero, zero, zero, zero
    normA2, maxrbar, minrbar = alpha * alpha, zero, T(1e100)
    normb, normAr = beta, alpha * beta
    it, istop = 0, 0
    limit = maxiter if iters is None else iters
    if normAr != 0:
        with np.errstate(invalid="ignore", divide="ignore"):
            while it < limit:
                it += 1
                uy, ux = A_v(v, alpha, uy, ux)
                beta = norm_u(uy, ux)
                if beta > 0:
                    uy, ux = uy * (one / beta), ux * (one / beta)
                    v = At_u(uy, ux, beta, v)
                    alpha = nrm(v)
                    if alpha > 0:
                        v = v * (one / alpha)
                alphahat = alphabar                      # lambda = 0: chat = 1, shat = 0
                rhoold = rho
                rho = np.sqrt(alphahat * alphahat + beta * beta)
                c, sn = alphahat / rho, beta / rho
                thetanew = sn * alpha
                alphabar = c * alpha
                rhobarold, zetaold = rhobar, zeta
                thetabar, rhotemp = sbar * rho, cbar * rho
                rhobar = np.sqrt((cbar * rho) * (cbar * rho) + thetanew * thetanew)
                cbar = cbar * rho / rhobar
                sbar = thetanew / rhobar
                zeta = cbar * zetabar
                zetabar = -sbar * zetabar
                hbar = hbar * (-thetabar * rho / (rhoold * rhobarold)) + h
                x = x + (zeta / (rho * rhobar)) * hbar
                h = h * (-thetanew / rho) + v
                betaacute = betadd
                betahat = c * betaacute
                betadd = -sn * betaacute
                thetatildeold = thetatilde
                rhotildeold = np.sqrt(rhodold * rhodold + thetabar * thetabar)
                ctildeold, stildeold = rhodold / rhotildeold, thetabar / rhotildeold
                thetatilde = stildeold * rhobar
                rhodold = ctildeold * rhobar
                betad = -stildeold * betad + ctildeold * betahat
                tautildeold = (zetaold - thetatildeold * tautildeold) / rhotildeold
                taud = (zeta - thetatilde * tautildeold) / rhodold
                normr = np.sqrt(d + (betad - taud) * (betad - taud) + betadd * betadd)
                normA2 = normA2 + beta * beta
                normA = np.sqrt(normA2)
                normA2 = normA2 + alpha * alpha
                maxrbar = max(maxrbar, rhobarold)
                if it > 1:
                    minrbar = min(minrbar, rhobarold)
                condA = max(maxrbar, rhotemp) / min(minrbar, rhotemp)
                normAr = abs(zetabar)
                normx = nrm(x)
                q = dict(alpha=alpha, beta=beta, normr=normr, normAr=normAr, normx=normx, normA=normA, condA=condA,
                         test1=normr / normb, test2=normAr / (normA * normr), test3=one / condA)
                q["t1"] = q["test1"] / (one + normA * normx / normb)
                q["rtol"] = btol + atol * normA * normx / normb
                q["x"] = P * x
                q["fired"] = rules_that_hold(q, it, maxiter, atol, ctol, one)
                rec.its.append(q)
                if iters is None and q["fired"]:
                    istop = q["fired"][0]
                    break
    rec.iter, rec.istop = it, istop
    rec.x = P * x
    return rec


def margins(rec, atol=ATOL, ctol=1.0 / CONLIM):
    """How far every rule is from its threshold, from the record of a solve run with the rules on.  Returns (passed, missed):
    `passed` = threshold / quantity of the rule that stopped the solve (None unless istop is 1, 2 or 3);
    `missed` = the smallest quantity / threshold over rules 1 to 6 wherever a rule was tried and did not hold: all of them at
    every earlier iteration and, at the stopping iteration, those tried BEFORE the one that fired (the ones behind it cannot
    change istop; nothing is tried before rule 7).  The round-off rules 4, 5, 6 hold when their quantity is <= 2^-53."""
    passed, missed = None, np.inf
    unit = 2.0 ** -53
    for k, q in enumerate(rec.its):
        last = k == len(rec.its) - 1
        thr = {1: (q["test1"], q["rtol"]), 2: (q["test2"], atol), 3: (q["test3"], ctol),
               4: (q["t1"], unit), 5: (q["test2"], unit), 6: (q["test3"], unit)}
        for rule, (val, t) in thr.items():
            val, t = float(val), float(t)
            if last and rule == rec.istop:
                if rule <= 3:
                    passed = t / val if val > 0 else np.inf
            elif last and (rec.istop == 7 or rule < rec.istop):
                continue
            elif not np.isnan(val):
                missed = min(missed, val / t)
    return passed, missed
