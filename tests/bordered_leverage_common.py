"""Shared by tests/test_bordered_leverage_host.py (no device) and tests/test_z_gpu_bordered_leverage.py: the cases, the longdouble
reference, the fp64 e_ref and the numpy fp64 twin of lsq_bordered_qr_leverage (lsq_lev_bordered.hip).

The rule is the accuracy tier's, unchanged: ac.judge, e_dev <= 16 max(e_ref, min(max(16, k), 64) 2^-53) with k = nb + ng, in
the metric of leverage_common: e(q) = max_i |q_i - q_hp,i| / q_hp,i (se: the same on sqrt(s2 q)).
    cases  borderedqr_cov_common.CASES, and plain (1, 2, 1, 1) for m = n
    q_hp   leverage_common.q_hp on J.toarray() (longdouble Householder, X = inv(R), row sums of squares of A X); a
           column-scaled handle: on V diag(s) in longdouble
    e_ref  leverage_common.q_fp64 on J.toarray() (LAPACK's Householder R, a triangular solve)
Neither comes from the code under test.

The twin follows the device steps in fp64: borderedqr_common.eliminate_block with zero damping per block, a pivoted LAPACK QR
of the F stack (F P = Q_g R_g), X_g = inv(R_g), and per row with local part a_b and shared part c
    z = inv(R_b)' a_b      e = c - W_b' z      u = X_g' P' e      q = ||z||^2 + ||u||^2
PLANTS are mistakes the rule must catch."""
import functools

import numpy as np
import scipy.linalg

import accuracy_common as ac
import borderedqr_common as bqc
import borderedqr_cov_common as bc
import hp_reference as hp
import leverage_common as lc

SQUARE = ("plain", (1, 2, 1, 1))                # m = n: every leverage is 1, no variance
CASES = list(bc.CASES) + [SQUARE]
PLANTS = ("no-border-term", "sign", "no-inner-permutation", "no-colscale")
case_id = bc.case_id


@functools.lru_cache(maxsize=None)
def operand(family, shape):
    if (family, shape) == SQUARE:
        return ac.bb_operand(family, *shape, 4242)
    return bc.operand(family, shape)


def full_rows(J, b, A_local, A_shared):
    """The p x n rows whose local part belongs to block b."""
    B, nb, ng = J.nblocks, J.nb, J.ng
    A = np.zeros((A_local.shape[0], B * nb + ng), order="F")
    A[:, b * nb:(b + 1) * nb] = A_local
    A[:, B * nb:] = A_shared
    return A


class Ref:
    """One operand with the longdouble and the fp64 quadratic forms of the rows A (None: J's own).  scaled: the handle holds
    op.V and means V diag(s) unrounded; the fp64 comparator works on J = fl(V diag(s))."""

    def __init__(self, op, scaled=False, A=None):
        J = op.J
        self.B, self.mb, self.nb, self.ng = J.nblocks, J.mb, J.nb, J.ng
        self.m, self.n = J.shape
        self.k = self.nb + self.ng
        self.A = J.toarray()
        eff = (hp.ld(op.V.toarray()) * hp.ld(op.s)) if scaled else self.A
        self.f = op.y
        self.q_hp = lc.q_hp(eff, A)
        self.q_ref = lc.q_fp64(self.A, A)
        dof = self.m - self.n
        self.s2_hp = ac.s2_of(op.y, dof) if dof > 0 else None
        self.s2 = float(op.y @ op.y) / dof if dof > 0 else None


@functools.lru_cache(maxsize=None)
def ref(family, shape, scaled=False):
    return Ref(operand(family, shape), scaled)


def pieces(name, q_dev, r, with_f=False, se_dev=None):
    """(name, e_dev, e_ref, k = nb + ng) of q against r.q_hp / r.q_ref and, with_f, of se against sqrt(s2 q)."""
    out = [(name, lc.lev_err(q_dev, r.q_hp), lc.lev_err(r.q_ref, r.q_hp), r.k)]
    if with_f:
        se_hp = np.sqrt(r.s2_hp * r.q_hp)
        se_ref = np.sqrt(r.s2 * r.q_ref)
        out.append((name + " se", lc.lev_err(se_dev, se_hp), lc.lev_err(se_ref, se_hp), r.k))
    return out


def judge(label, pcs):
    ac.judge(label, pcs)


def beyond(pcs):
    """The largest e / bound over the pieces: > 1 means outside the rule."""
    return bqc.beyond(pcs)


def new_rows(J, b, p, seed):
    """p rows of block b drawn like the operand's own: rows of [J_b | C_b] picked at random, each times a random factor."""
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, J.mb, p)
    fac = 1.0 + 0.5 * rng.standard_normal((p, 1))
    return np.asfortranarray(J.block(b)[pick] * fac), np.asfortranarray(J.border_block(b)[pick] * fac)


# ------------------------------------------------------------------------------------------ the twin
class Factor:
    """The factor the entry point keeps on the device, in fp64: per block R_b, W_b; X_g = inv(R_g) and the pivots of F."""

    def __init__(self, J, colscale=None):
        B, mb, nb, ng = J.nblocks, J.mb, J.nb, J.ng
        self.J, self.B, self.mb, self.nb, self.ng = J, B, mb, nb, ng
        self.s = np.ones(B * nb + ng) if colscale is None else np.asarray(colscale, dtype=np.float64)
        sg = self.s[B * nb:]
        self.R, self.W, Fs = [], [], []
        for b in range(B):
            R, W, _, F, _, bad = bqc.eliminate_block(J.block(b) * self.s[b * nb:(b + 1) * nb], J.border_block(b) * sg,
                                                     np.zeros(mb), np.zeros(nb))
            assert bad == 0
            self.R.append(R)
            self.W.append(W)
            Fs.append(F)
        Rg, self.P = scipy.linalg.qr(np.vstack(Fs), mode="r", pivoting=True)
        self.Xg = scipy.linalg.solve_triangular(np.triu(Rg[:ng, :ng]), np.eye(ng), lower=False)

    def q(self, b, A_local, A_shared, plant=None):
        """The quadratic forms of rows of block b that are in the parameter space the handle means."""
        Z = scipy.linalg.solve_triangular(self.R[b], np.asarray(A_local).T, trans="T", lower=False).T
        ZW = Z @ self.W[b]
        E = A_shared + ZW if plant == "sign" else A_shared - ZW
        U = (E if plant == "no-inner-permutation" else E[:, self.P]) @ self.Xg
        qz = np.sum(Z * Z, axis=1)
        return qz if plant == "no-border-term" else qz + np.sum(U * U, axis=1)

    def own(self, plant=None):
        """J's own rows: staged with the handle's column scale, as k_bl_local does."""
        B, nb = self.B, self.nb
        sg = self.s[B * nb:]
        out = []
        for b in range(B):
            Ab, Cb = self.J.block(b), self.J.border_block(b)
            if plant != "no-colscale":
                Ab, Cb = Ab * self.s[b * nb:(b + 1) * nb], Cb * sg
            out.append(self.q(b, Ab, Cb, plant))
        return np.concatenate(out)


def twin(J, colscale=None, plant=None):
    return Factor(J, colscale).own(plant)


def q_normal_equations(A, rows=None):
    """The route the entry point avoids, all fp64; inf where inv(J'J) cannot be formed."""
    try:
        return lc.q_normal_equations(A, rows)
    except np.linalg.LinAlgError:
        return np.full((A if rows is None else rows).shape[0], np.inf)
