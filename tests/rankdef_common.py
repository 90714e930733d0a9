"""Rank-deficient operands for the accuracy tier: builders, longdouble references, metrics and case lists shared by
tests/test_rankdef_host.py (no device) and tests/test_s_gpu_accuracy_rankdef.py.  The rule is tests/accuracy_common.py's
(ac.judge: e_dev <= 16 max(e_ref, min(max(16, k), 64) 2^-53)); the references are tests/hp_reference.py's.

Family E -- exact rank, a reference that knows nothing of pivoting or rank decisions
    A = (B C) D, B (m x r) and C (r x n) integers from [-3, 3], D a diagonal of powers of two spread over 0 / 4 / 8 decades and
    shuffled over the columns (8 decades: n <= 64 only).  Every entry of A is an integer times a power of two, exact in fp64
    (asserted in the builder: the fp64 product against the exact one, formed from the int64 product of the factors and D in
    longdouble).  rank(A) = r exactly, and the minimum-norm least-squares solution is x_hp = (C D)^+ B^+ y:
    hp.minnorm_from_factors -- hp.lstsq_qr for B^+ y, a Householder QR of (C D)' for the rest (NOT the Cholesky factor of
    (C D)(C D)': with D over 8 decades cond(C D)^2 reaches 1e13 .. 1e16, and 2^-64 times that is no longer below LAPACK's own
    error, 7e-8; test_rankdef_host.py holds the two forms together where the Gram matrix is benign).
    Variants: dup / dup4 -- column 0 once more in the last column (a tie in the pivot search; the minimum-norm solution does not
    depend on how it is broken), on plain and on 4 decades; zero1 / zero2 -- one / two all-zero columns; far+ / far- -- A and y
    times 2^+-100 (rank and every bit of x_hp unchanged).
    metric   e(x) = ||x - x_hp||_2 / ||x_hp||_2, a plain norm (a minimum-norm solution is not invariant under column scaling)
    e_ref    the same for the oracle, O.qr_solve (geqp3 + xGELSY)
Family T -- rank decided near the threshold
    A = U diag(sigma) V', sigma_1..r = logspace(0, log10(K rcond), r), sigma_(r+1..) = rcond / K, rcond = min(m, n) eps,
    K = 30 and 1000; r = min(m, n): just full rank.  x is good to cond(R11) u only, so the residual is judged:
    rho(x) = ||A x - y||_2 / (||A||_F ||x||_2 + ||y||_2), against rho_hp of hp.pivoted_truncated_solve with the oracle's pivots and
    rank: |rho_dev - rho_hp| <= 16 max(|rho_orc - rho_hp|, 64 * 2^-53)   (t_bound; ac.bound with k = 64)
Family Z -- LM's stacked operand, itself rank-deficient
    a family-E operand with r = n and z of its columns zeroed, damp = 0.1 colsumabs2(A): exactly 0 on those columns, so
    [A; diag(sqrt(damp))] has z all-zero columns.  Reference: x_j = 0 there, hp.lstsq_qr of the stacked longdouble operand
    restricted to the other columns; metric ac.solve_err with S = the column norms of A on those columns; e_ref O.ldiv(O.QR, ..).
Beyond 400 columns the Householder forms in longdouble take a quarter of a minute each, so there B^+ y, (C D)^+ z (unscaled
variants only) and the damped solve come from Gram matrices formed EXACTLY from the integer factors, a longdouble Cholesky
factor and one refinement step (hp.normal_solve_refined, hp.minnorm_gram_refined; held against the Householder forms in
tests/test_rankdef_host.py), and the oracle's geqp3 is served by LAPACK's dgeqp3 beyond 512 columns (O.use_lapack_geqp3).

Every seed is a function of the shape, written down here before the first device run.  Where a factor is square or nearly
so, the draw is repeated (seed + 1000, + 2000, ..) until both factors have cond <= 1e3 in fp64 numpy: a property of the
operand alone."""
import functools

import numpy as np

import accuracy_common as ac
import hp_reference as hp
from oracle import oracle as O

LD = hp.LD
EPS = float(np.finfo(float).eps)
COND_MAX = 1e3
FAR = {"far+": 2.0 ** 100, "far-": 2.0 ** -100}
DECADES = {"plain": 0, "dec4": 4, "dec8": 8, "dup": 0, "dup4": 4, "zero1": 0, "zero2": 0, "far+": 0, "far-": 0}

# ------------------------------------------------------------------------------------------ shapes per device path
ONE_WG = [(30, 12, 7), (9, 6, 5), (20, 8, 1), (6, 10, 4), (40, 33, 20)]
ONE_STAGE = [(700, 100, 37), (1100, 130, 129), (300, 256, 1), (80, 900, 60)]        # 80 x 900: M < n, k_qrcp_solve's own phases
TWO_STAGE = [(900, 100, 37), (700, 200, 1), (1000, 321, 300), (900, 800, 700)]      # 321: k_qr2_step<2>; 800: <4>
SWEEP = (2100, 2049, 5)                                                             # n > 2048: k_qr_norms / pivot / apply on R
ENV = {"one-workgroup": {}, "one-stage": {"LSQ_QR_ONE_STAGE": "1"}, "two-stage": {"LSQ_QR_TWO_STAGE": "1"},
       "sweep": {"LSQ_QR_TWO_STAGE": "1"}}
QR_PATH = {"one-workgroup": "one-stage", "one-stage": "one-stage", "two-stage": "two-stage-pivoted", "sweep": "two-stage-pivoted"}


def multi_cu(M, n):
    """lsq_qr_solve: the two-launch-per-column kernels once the two-stage path is off; below it k_qrcp_solve alone."""
    return n >= 64 and M * n >= 65536


def two_stage_by_default(M, n):
    """qr2_applies without a switch."""
    return M >= n and n >= 2 and ((n >= 16 and M * n >= 1600) or M * n >= 20000)


def e_variants(m, n, r, wanted):
    """The variants of `wanted` that leave rank r possible: a duplicate needs n - 1 >= r, z zero columns n - z >= r (and a
    column beside them to stay interesting); 8 decades n <= 64."""
    out = []
    for v in wanted:
        if v == "dec8" and n > 64:
            continue
        if v in ("dup", "dup4") and n - 1 < r:
            continue
        if v == "zero1" and n - 1 < r:
            continue
        if v == "zero2" and n - 2 < r:
            continue
        out.append(v)
    return out


ALL_VARIANTS = ("plain", "dec4", "dec8", "dup", "dup4", "zero1", "zero2", "far+", "far-")
E_CASES = ([("one-workgroup", m, n, r, v) for (m, n, r) in ONE_WG for v in e_variants(m, n, r, ALL_VARIANTS)] +
           [("one-stage", 700, 100, 37, v) for v in e_variants(700, 100, 37, ALL_VARIANTS)] +
           [("one-stage", 1100, 130, 129, v) for v in ("plain", "dec4", "dup", "zero1")] +
           [("one-stage", 300, 256, 1, v) for v in ("plain", "dec4", "zero2", "far-")] +
           [("one-stage", 80, 900, 60, v) for v in ("plain", "dec4", "dup", "far+")] +
           [("two-stage", 900, 100, 37, v) for v in e_variants(900, 100, 37, ALL_VARIANTS)] +
           [("two-stage", 700, 200, 1, v) for v in ("plain", "dec4", "zero2")] +
           [("two-stage", 1000, 321, 300, v) for v in ("plain", "dec4", "dup")] +
           [("two-stage", 900, 800, 700, "plain")] +                     # (the exact-Gram reference: unscaled only)
           [("two-stage", 900, 800, 20, v) for v in ("dec4", "dup4")])  # mixed scales and a tie in k_qr2_step<4>
E_SWEEP_CASE = ("sweep",) + SWEEP + ("dec4",)
E_DEFAULT_CASES = [(30, 12, 7, "dec4", "one-stage"), (900, 100, 37, "dup4", "two-stage-pivoted")]      # no switch at all

# family T: one shape per path, deficient and just full rank, K = 30 and 1000 (the sweep: K = 30, deficient)
T_SHAPES = {"one-workgroup": (40, 33, 20), "one-stage": (700, 100, 37), "two-stage": (900, 100, 37)}
T_CASES = [(p, m, n, rr, K) for p, (m, n, r) in T_SHAPES.items() for rr in (r, n) for K in (30, 1000)]
T_SWEEP_CASE = ("sweep",) + SWEEP + (30,)

# family Z: the shapes above with m >= n (the stacked operand is (m + n) x n), z = 1 and 3; 0 and 4 decades alternate.  Not at
# 2100 x 2049: a longdouble solve of the stacked 4149 x 2046 operand takes most of a minute in either form
Z_SHAPES = ([("one-workgroup", m, n) for (m, n, _) in ONE_WG if m >= n] + [("one-stage", m, n) for (m, n, _) in ONE_STAGE if m >= n] +
            [("two-stage", m, n) for (m, n, _) in TWO_STAGE])
Z_CASES = [(p, m, n, z, ("plain", "dec4")[(i + z // 2) % 2]) for i, (p, m, n) in enumerate(Z_SHAPES) for z in (1, 3)]

BQ_NBS = (5, 16, 17, 33, 64)
BQ_MBS = (3, 40, 257)


# ------------------------------------------------------------------------------------------ family E
def e_seed(m, n, r):
    return 500000 + 1000 * m + 7 * n + r


def _cond(M):
    s = np.linalg.svd(M.astype(np.float64), compute_uv=False)
    return np.inf if s[-1] == 0 else float(s[0] / s[-1])


def _draw_by(m, r, seed):
    """B and y: functions of (m, r, seed) alone, so that every variant of a shape shares z = B^+ y."""
    rng = np.random.default_rng(seed)
    return rng, rng.integers(-3, 4, size=(m, r)), rng.standard_normal(m)


def scale_exponents(n, decades, perm):
    """D = 2^e: e spread evenly from 0 down to -decades * log2(10) (rounded), then shuffled over the columns."""
    if decades == 0 or n == 1:
        return np.zeros(n, dtype=np.int64)
    e = -np.rint(np.arange(n) * (decades * np.log2(10.0) / (n - 1))).astype(np.int64)
    return e[perm]


class EOperand:
    """A (fp64, column-major), y, the factors B (m x r, int64), C (r x n, int64, the variant's: duplicate / zero columns in
    place) and W = C D (longdouble, exact), the intended rank.  certify: repeat the draw until cond(B), cond(C) <= 1e3
    (default: where a factor is square or nearly so; further out a random integer factor is far below it, and
    tests/test_rankdef_host.py asserts it of every committed case either way)."""

    def __init__(self, m, n, r, variant, seed=None, certify=None, zero_cols=None):
        self.m, self.n, self.r, self.variant = m, n, r, variant
        seed = e_seed(m, n, r) if seed is None else seed
        certify = (r >= 0.75 * min(m, n)) if certify is None else certify
        if zero_cols is None:
            zero_cols = {"zero1": [1], "zero2": [1, n - 2]}.get(variant, [])
        self.zero_cols = sorted(zero_cols)
        for attempt in range(40):
            self.seed = seed + 1000 * attempt
            rng, B, y = _draw_by(m, r, self.seed)
            C = rng.integers(-3, 4, size=(r, n))
            perm = rng.permutation(n)
            if variant in ("dup", "dup4"):
                C[:, n - 1] = C[:, 0]
            C[:, self.zero_cols] = 0
            if not certify or (_cond(B) <= COND_MAX and _cond(C) <= COND_MAX):
                break
        else:
            raise AssertionError(("no well-conditioned factors", m, n, r, seed))
        d = 2.0 ** scale_exponents(n, DECADES[variant], perm)
        if variant in ("dup", "dup4"):
            d[n - 1] = d[0]
        self.B, self.C, self.d = B, C, d
        P = B @ C                                           # int64: exact
        A = (B.astype(np.float64) @ C.astype(np.float64)) * d
        assert np.max(np.abs(P)) < 2 ** 53 and np.array_equal(hp.ld(A), P.astype(LD) * hp.ld(d)), "A = (B C) D is not exact in fp64"
        self.P = P
        self.f = FAR.get(variant, 1.0)
        self.A = np.asfortranarray(A * self.f)
        self.y = y * self.f
        self.y0 = y                                         # unscaled: x_hp has the same bits
        self.W = hp.ld(C) * hp.ld(d)

    def factor_conds(self):
        return _cond(self.B), _cond(self.C)


GRAM_FROM = 400         # factors with more columns / rows than this take the exact-Gram forms of hp_reference
GRAM_COND_MAX = 100.0   # ... which square the condition number: 1e4 * 2^-64, squared once more by the refinement step


@functools.lru_cache(maxsize=4)
def _e_z(m, r, seed):
    """z = B^+ y in longdouble, shared by every variant of the shape.  hp.lstsq_qr; for r > 400 (a quarter of a minute there)
    the normal equations with the EXACT integer Gram matrix B'B and one refinement step, B being far from ill-conditioned."""
    _, B, y = _draw_by(m, r, seed)
    if r <= GRAM_FROM:
        return hp.lstsq_qr(B, y)
    assert _cond(B) <= GRAM_COND_MAX
    return hp.normal_solve_refined(B, y, (B.T @ B).astype(LD))


def e_x_hp(op):
    z = _e_z(op.m, op.r, op.seed)
    if op.r <= GRAM_FROM:
        return hp.minnorm_solve(op.W, z)
    assert np.all(op.d == 1.0) and _cond(op.C) <= GRAM_COND_MAX, "the exact-Gram form is for unscaled, well-conditioned C"
    return hp.minnorm_gram_refined(op.W, z, (op.C @ op.C.T).astype(LD))


def rel_err(x, x_hp):
    x, x_hp = hp.ld(x), hp.ld(x_hp)
    d = x - x_hp
    return float(np.sqrt(d @ d) / np.sqrt(x_hp @ x_hp))


LAPACK_GEQP3_FROM = 512


def oracle_with_lapack_geqp3(n, call):
    """Run `call` with the oracle's geqp3 served by LAPACK's dgeqp3 when n > 512 (O.use_lapack_geqp3: the scalar restatement
    needs seconds at 900 x 800 and most of a minute at 2100 x 2049); everything after the factorisation stays the oracle's."""
    big = n > LAPACK_GEQP3_FROM
    if big:
        O.use_lapack_geqp3(True)
    try:
        return call()
    finally:
        if big:
            O.use_lapack_geqp3(False)


def oracle_solve(A, y, rcond=None):
    """(x, rank, jpvt) of O.qr_solve."""
    x, rk, jp, *_ = oracle_with_lapack_geqp3(A.shape[1], lambda: O.qr_solve(A, y, rcond=rcond))
    return x, int(rk), np.array(jp)


def lapack_gelsy(A, y, rcond=None):
    """(x, rank) of LAPACK's own dgelsy (blocked dgeqp3): a second realisation of the reference's algorithm."""
    from scipy.linalg import lstsq
    x, _, rank, _ = lstsq(np.asarray(A), y, cond=min(A.shape) * EPS if rcond is None else rcond, lapack_driver="gelsy")
    return x, int(rank)


class ERef:
    def __init__(self, m, n, r, variant):
        self.op = EOperand(m, n, r, variant)
        self.x_hp = e_x_hp(self.op)
        self.x_orc, self.rank_orc, self.jpvt = oracle_solve(self.op.A, self.op.y)
        self.e_ref = rel_err(self.x_orc, self.x_hp)


@functools.lru_cache(maxsize=4)
def e_ref(m, n, r, variant):
    return ERef(m, n, r, variant)


# ------------------------------------------------------------------------------------------ family T
def t_seed(m, n, r, K):
    return 700000 + 1000 * m + 7 * n + 3 * r + K


def t_matrix(rng, m, n, r, K):
    k = min(m, n)
    rcond = k * EPS
    U, _ = np.linalg.qr(rng.standard_normal((m, k)))
    V, _ = np.linalg.qr(rng.standard_normal((n, k)))
    s = np.full(k, rcond / K)
    s[:r] = np.logspace(0, np.log10(K * rcond), r)
    return np.asfortranarray((U * s) @ V.T)


def rho(A, x, y):
    A, x, y = hp.ld(A), hp.ld(x), hp.ld(y)
    res = A @ x - y
    return np.sqrt(res @ res) / (np.sqrt(np.sum(A * A)) * np.sqrt(x @ x) + np.sqrt(y @ y))


def t_bound(rho_orc, rho_hp):
    return ac.bound(abs(float(rho_orc - rho_hp)), ac.FLOOR_CAP)


class TRef:
    """One family-T problem: the oracle's rank / pivots / solution, the longdouble solution for those pivots and that rank,
    both residuals.  accepts(x): the rule."""

    def __init__(self, A, y, r):
        self.A, self.y, self.r = A, y, r
        self.x_orc, self.rank_orc, self.jpvt = oracle_solve(A, y)
        self.x_hp = hp.pivoted_truncated_solve(A, y, self.jpvt, self.rank_orc)
        self.rho_hp, self.rho_orc = rho(A, self.x_hp, y), rho(A, self.x_orc, y)
        self.bound = t_bound(self.rho_orc, self.rho_hp)

    def dist(self, x):
        return abs(float(rho(self.A, x, self.y) - self.rho_hp))

    def accepts(self, x):
        d = self.dist(x)
        return bool(np.isfinite(d)) and d <= self.bound

    def judge(self, label, x):
        d = self.dist(x)
        print("ACC %s | rho_hp %.6e |rho_dev - rho_hp| %.3e |rho_orc - rho_hp| %.3e ratio %.2f bound %.3e"
              % (label, float(self.rho_hp), d, abs(float(self.rho_orc - self.rho_hp)),
                 d / max(abs(float(self.rho_orc - self.rho_hp)), 1e-300), self.bound))
        assert np.isfinite(d) and d <= self.bound, (label, d, self.bound)


@functools.lru_cache(maxsize=4)
def t_ref(m, n, r, K):
    rng = np.random.default_rng(t_seed(m, n, r, K))
    A = t_matrix(rng, m, n, r, K)
    return TRef(A, rng.standard_normal(m), r)


# ------------------------------------------------------------------------------------------ family Z
def z_env(path, m, n):
    """The switches of a family-Z case: the stacked (m + n) x n operand of a one-workgroup shape may be large enough for the
    default dispatch to take the two-stage path (73 x 33); LSQ_QR_ONE_STAGE keeps it on k_qrcp_solve."""
    if path == "one-workgroup" and two_stage_by_default(m + n, n):
        return {"LSQ_QR_ONE_STAGE": "1"}
    return ENV[path]


def z_cols(n, z):
    return [1] if z == 1 else [0, n // 2, n - 1]


class ZRef:
    """Damped problem on an operand with zero columns: keep = the other columns; x_hp (0 on the zero columns); the oracle's
    damped solve, its rank (the same factorisation once more, as tests/test_e_gpu_blockqr.py::oracle_blocks) and e_ref."""

    def __init__(self, A, y, gram=None):
        n = A.shape[1]
        self.A, self.y, self.n = A, y, n
        self.damp = 0.1 * ac.colsumabs2(A)
        self.keep = np.flatnonzero(np.any(A != 0, axis=0))
        assert np.all(self.damp[self.keep] > 0) and np.all(np.delete(self.damp, self.keep) == 0.0)
        self.x_hp = np.zeros(n, dtype=LD)
        if len(self.keep):
            if gram is None:
                As, ys = ac.stacked(hp.ld(A[:, self.keep]), hp.ld(y), self.damp[self.keep])
                self.x_hp[self.keep] = hp.lstsq_qr(As, ys)
            else:       # (n > 400: the damped normal equations are the same problem, and well-conditioned at damp = 0.1 colsumabs2)
                self.x_hp[self.keep] = hp.normal_solve_refined(A[:, self.keep], y, gram[np.ix_(self.keep, self.keep)], self.damp[self.keep])
        self.S = ac.colnorms(A[:, self.keep])
        st, self.x_orc, nmul, d_after = oracle_with_lapack_geqp3(
            n, lambda: O.ldiv(O.QR, O.Mat(dense=np.asfortranarray(A)), y, self.damp))
        assert st == 0 and nmul == 1 and np.array_equal(d_after, self.damp)
        As64, ys64 = ac.stacked(np.asarray(A), y, self.damp)
        _, self.rank_orc, _ = oracle_solve(As64, ys64, rcond=n * EPS)
        self.e_ref = self.err(self.x_orc) if len(self.keep) else 0.0

    def err(self, x):
        return ac.solve_err(np.asarray(x)[self.keep], self.x_hp[self.keep], self.S)


@functools.lru_cache(maxsize=2)
def z_ref(m, n, z, variant):
    op = EOperand(m, n, n, variant, seed=e_seed(m, n, n) + 1, certify=False, zero_cols=z_cols(n, z))
    gram = None
    if n > GRAM_FROM:       # A'A = D (P'P) D, P = B C integer: exact in longdouble (P'P < 2^63, D powers of two)
        gram = (op.P.T @ op.P).astype(LD) * np.outer(hp.ld(op.d), hp.ld(op.d))
        assert np.max(np.abs(op.P)) ** 2 * m < 2 ** 62
    return ZRef(op.A, op.y, gram)


# ------------------------------------------------------------------------------------------ BlockQR batches
class Block:
    def __init__(self, kind, A, y, rank, x_hp=None, tref=None, decades=0):
        self.kind, self.A, self.y, self.rank, self.x_hp, self.tref, self.decades = kind, A, y, rank, x_hp, tref, decades


def bq_seed(mb, nb, b):
    return 900000 + 1000 * mb + 10 * nb + b


@functools.lru_cache(maxsize=2)
def bq_batch(mb, nb):
    """Nine blocks: E deficient (plain, 4 and 8 decades), E full rank (plain, 4 decades), a duplicated column, a zero column,
    one all-zero block, one family-T block (K = 30).  Undamped references per block; damped ones: bq_damped_refs."""
    k = min(mb, nb)
    r1, r2, rt = max(1, k // 2), max(1, k - 1), max(2, k // 2 + 1)
    spec = [("E deficient", r1, "plain"), ("E full", k, "plain"), ("E deficient", r2, "dec4"), ("E dup", r1, "dup"),
            ("E zero", r2, "zero1"), ("zero", 0, None), ("E deficient", r1, "dec8"), ("T", rt, None), ("E full", k, "dec4")]
    blocks = []
    for b, (kind, r, variant) in enumerate(spec):
        seed = bq_seed(mb, nb, b)
        if kind == "zero":
            y = np.random.default_rng(seed).standard_normal(mb)
            blocks.append(Block(kind, np.zeros((mb, nb), order="F"), y, 0, x_hp=np.zeros(nb, dtype=LD)))
        elif kind == "T":
            rng = np.random.default_rng(seed)
            A = t_matrix(rng, mb, nb, r, 30)
            y = rng.standard_normal(mb)
            blocks.append(Block(kind, A, y, r, tref=TRef(A, y, r)))
        else:
            op = EOperand(mb, nb, r, variant, seed=seed, certify=True)
            blocks.append(Block(kind, op.A, op.y, r, x_hp=hp.minnorm_from_factors(op.B, op.W, op.y), decades=DECADES[variant]))
    return blocks


@functools.lru_cache(maxsize=2)
def bq_damped_refs(mb, nb):
    return [ZRef(blk.A, blk.y) for blk in bq_batch(mb, nb)]
