"""Handle state tier, shared part (tests/test_handle_state_host.py, tests/test_t_gpu_handle_state.py): the Jacobian handle as a
state machine.  An lsq_mat keeps its values in up to five layouts, two colsum caches and three flags, and which copy is the
authority changes with the last mutation (include/lsqhip.h, "FRESHNESS CONTRACT").  This module holds, WITHOUT touching a
device (the library is only handed in by the GPU file):

  * CONFIGS: the layout configurations -- natural ones (no switch: what lsq_csc_create picks by itself at the smallest shapes
    that still select it), forced ones (the switches of tests/test_i_gpu_accuracy_products.py's LAYOUTS on 3000 x 200, also
    with LSQ_NO_COLSCALE=1), and "g:" ones whose handle belongs to the built-in tanh model (lsq_model_g is then a mutation);
  * Twin: a numpy object with the stored values V, the scale s or None and the pattern; every mutation has a twin method, every
    reader a reference in longdouble (products), fp64 (sums, Gram) or LAPACK (solves, covariance);
  * sequences(): per configuration S sequences of L steps from fixed seeds; a step is one mutation and two readers, the last
    step runs all readers.  A greedy walk that prefers what is not yet covered; the host file asserts that every ordered
    (mutation, reader) pair and every ordered legal (mutation, mutation) pair occurs;
  * judge(): oracle 2, the independent reference.  Bounds: products by accuracy_common.judge_product with the counts of
    test_i (c = 3, 4 with a scale); column / row sums rtol 1e-13 (test_b); direct solves and covariances normwise 1e-9
    (gpu_common); LSMR as gpu_common states it -- identical product count and rel 1e-8 against the CPU oracle's LSMR on the
    twin's effective matrix (its stopping rule, atol 1e-6, ends long before 1e-9 of the LAPACK solution, so lstsq is the
    reference of the direct solvers only); values() exactly V.
    Gram (no earlier tolerance exists): entry (k, j) is a dot product of K_j stored terms, each a rounded product of two
    entries that a scale may have rounded once more: |G - ref| <= gamma_(K_j + 4) |E|'|E| for any order of summation; the fp64
    scipy reference carries the same bound, hence twice that.

Mutation names: set_values, async_wait, async_nowait (set_values_async from a pinned buffer, with / without upload_wait before
the next reader), write_refresh (device write through lsq_mat_values + lsq_mat_refresh), set_colscale (first), set_colscale_again
(another vector while one is set), s_inplace (rewrite s + colscale_changed), unscale (set_colscale(None) with a scale),
unscale_plain (without one), fd (fd_jacobian_ of a linear f; on a scaled handle the documented refusal: fd_refused), g
(lsq_model_g).  Every one multiplies every affected entry by a factor from [0.5, 0.8] or [1.25, 2]."""
import functools

import numpy as np
import scipy.sparse as sp

import accuracy_common as ac
import hp_reference as hp

LD = np.longdouble
ALPHA_BETA = ((1.5, -0.5), (-2.0, 0.25))
SEQ_LEN = 12


# ------------------------------------------------------------------------------------------------ patterns
def _with_holes(m, n, rows, cols):
    """Empty row 3, empty column 1, full row 5 (but for the empty column) -- the choice of ac.ragged_pattern."""
    keep = (rows != 3) & (cols != 1) & (rows != 5)
    rows, cols = rows[keep], cols[keep]
    full = np.array([j for j in range(n) if j != 1], dtype=np.int64)
    rows = np.concatenate([rows, np.full(full.size, 5, dtype=np.int64)])
    cols = np.concatenate([cols, full])
    S = sp.coo_matrix((np.ones(rows.size), (rows, cols)), shape=(m, n)).tocsc()
    S.sum_duplicates()
    S.sort_indices()
    return S


def per_row_pattern(m, n, k, seed):
    """k distinct columns in every row: a random start plus one of 16 fixed offset sets (mod n)."""
    rng = np.random.default_rng(seed)
    table = np.stack([np.sort(rng.choice(n, size=k, replace=False)) for _ in range(16)])
    start = rng.integers(0, n, size=m)
    pat = rng.integers(0, 16, size=m)
    cols = (start[:, None] + table[pat]) % n
    rows = np.repeat(np.arange(m, dtype=np.int64), k)
    return _with_holes(m, n, rows, cols.reshape(-1).astype(np.int64))


def stream_heads_pattern(n, m=589):
    """The ragged pattern of tests/test_m_gpu_stream_heads.py (case(n)): full row 5, rows 256..511 empty, the last row and the
    last column used; column 1 emptied here."""
    rng = np.random.default_rng(1000 + n)
    S = sp.random(m, n, density=min(1.0, 3.5 / n), format="lil", random_state=rng, data_rvs=rng.standard_normal)
    S[5, :] = rng.standard_normal(n)
    S[256:512, :] = 0
    S[m - 1, n - 1] = 1.25
    S[0, 0] = -0.75
    S[:, 1] = 0
    S = S.tocsc()
    S.eliminate_zeros()
    S.sort_indices()
    return S


def full_pattern(m, n):
    return sp.csc_matrix((np.ones(m * n), np.tile(np.arange(m), n), np.arange(n + 1) * m), shape=(m, n))


def block_pattern(B, mb, nb, ng=0):
    m = B * mb
    indptr = np.concatenate([np.arange(B * nb + 1) * mb, B * nb * mb + np.arange(1, ng + 1) * m])
    blocks = (np.repeat(np.arange(B), nb)[:, None] * mb + np.arange(mb)[None, :]).reshape(-1)
    indices = np.concatenate([blocks, np.tile(np.arange(m), ng)])
    return sp.csc_matrix((np.ones(indices.size), indices, indptr), shape=(m, B * nb + ng))


# ------------------------------------------------------------------------------------------------ configurations
class Config:
    """kind: csc / dense / block / bordered.  env: switches around creation (monkeypatch); nocolscale: LSQ_NO_COLSCALE=1 around
    creation and the first set_colscale.  model: the handle belongs to a TanhProblem (fused: the model scales through the
    handle's fused column scale).  expect: what layout() must say after creation; scale_mode: what it must say once a scale is
    set.  lsmr_path: the driver an LSMR solve on it takes."""

    def __init__(self, name, kind, shape, pattern, expect, scale_mode, lsmr_path=None, env=None, nocolscale=False, model=False,
                 fused=False, block=None, fd=True, lazy=False):
        self.name, self.kind, self.shape, self._pattern = name, kind, shape, pattern
        self.expect, self.scale_mode, self.lsmr_path = expect, scale_mode, lsmr_path
        self.env, self.nocolscale, self.model, self.fused, self.block, self.fd, self.lazy = (
            dict(env or {}), nocolscale, model, fused, block, fd, lazy)

    @property
    def pattern(self):
        return self._pattern()

    @property
    def solvers(self):
        return {"csc": ("lsmr",), "dense": ("lsmr", "cholesky", "qr"), "block": ("lsmr", "cholesky", "blockqr"),
                "bordered": ("lsmr", "cholesky", "schur")}[self.kind]

    @property
    def readers(self):
        r = ["values", "mul", "mul_t", "colsum", "rowsum"] + ["ldiv:" + s for s in self.solvers]
        if self.kind != "dense":
            r.append("gram")
        r.append("cov")
        if self.kind == "dense":
            r.append("cov_qr")
        return tuple(r)

    @property
    def mutations(self):
        """Every mutation name that can occur in this configuration (legality depends on the state: legal())."""
        if self.model:
            mu = ["g", "set_values", "async_wait", "async_nowait", "write_refresh", "unscale_plain"]
            return tuple(mu + (["unscale"] if self.fused else []))
        mu = ["set_values", "async_wait", "async_nowait", "write_refresh", "set_colscale", "set_colscale_again", "s_inplace",
              "unscale", "unscale_plain"]
        return tuple(mu + (["fd", "fd_refused"] if self.fd else []))

    def legal(self, mutation, scaled):
        if mutation in ("set_colscale_again", "s_inplace", "unscale", "fd_refused"):
            return scaled
        if mutation in ("set_colscale", "unscale_plain", "fd"):
            return not scaled
        return True                     # uploads, the device write and the model's g! take either state

    def after(self, mutation, scaled):
        """Whether a scale is set after the mutation."""
        if mutation in ("set_colscale", "set_colscale_again", "s_inplace", "fd_refused"):
            return True
        if mutation in ("unscale", "unscale_plain", "fd"):
            return False
        if mutation == "g":
            return self.fused or scaled
        return scaled


def _cached(fn, *a):
    return functools.lru_cache(maxsize=1)(lambda: fn(*a))


_OFF = dict(srows=False, scols=False)
_FORCED = _cached(lambda: _with_holes(3000, 200, *sp.random(3000, 200, density=0.01, format="coo",
                                                             random_state=np.random.default_rng(3200)).nonzero()))
_SLICED = _cached(per_row_pattern, 140000, 64, 8, 11)
_SEGMENTS = _cached(per_row_pattern, 2500, 300, 6, 12)
_WINDOWED = _cached(per_row_pattern, 140000, 40, 4, 13)
_ROWS_ONLY = _cached(per_row_pattern, 60000, 500, 20, 14)
_SMALL = _cached(stream_heads_pattern, 129)
_SLICED_EXPECT = dict(kind="csc", srows=True, scols=True, ncw=1)


def _configs():
    C = [
        Config("small", "csc", (589, 129), _SMALL, dict(kind="csc", nwin=0, **_OFF), "materialising", "reference-order"),
        Config("segments", "csc", (2500, 300), _SEGMENTS, dict(kind="csc", nwin=0, **_OFF), "materialising", "four-launch"),
        Config("windowed", "csc", (140000, 40), _WINDOWED, dict(kind="csc", windowed=True, **_OFF), "materialising"),
        # 2 x 500 evaluations of f on 60000 rows per Jacobian: fd stays with the configurations where it takes milliseconds
        Config("rows-only", "csc", (60000, 500), _ROWS_ONLY, dict(kind="csc", srows=True, scols=False, ncw=1, nwin=0),
               "materialising", fd=False),
        Config("sliced", "csc", (140000, 64), _SLICED, _SLICED_EXPECT, "fused", "three-launch"),
        Config("dense-small", "dense", (300, 17), _cached(full_pattern, 300, 17), dict(kind="dense"), "materialising",
               "reference-order"),
        Config("dense", "dense", (2100, 40), _cached(full_pattern, 2100, 40), dict(kind="dense"), "materialising"),
        Config("block", "block", (360, 45), _cached(block_pattern, 9, 40, 5), dict(kind="csc", **_OFF), "materialising",
               "reference-order", block=(9, 40, 5)),
        Config("bordered", "bordered", (360, 52), _cached(block_pattern, 9, 40, 5, 7), dict(kind="csc", **_OFF), "materialising",
               "reference-order", block=(9, 40, 5, 7)),
    ]
    forced = {"sliced 64 64": ({"LSQ_SELL_FORCE": "1", "LSQ_SELL_ROWS": "64", "LSQ_SELL_GROWS": "64"},
                               dict(kind="csc", srows=True, scols=True, ncw=1, wrows=64, ngw=47)),
              # (LSQ_SELL_FORCE also lets the column windows through: wide_ok in lsq_csc_create, no LSQ_SELL_WIDE needed)
              "sliced xmax 64": ({"LSQ_SELL_FORCE": "1", "LSQ_SELL_XMAX": "64"},
                                 dict(kind="csc", srows=True, scols=True, ncw=4)),
              "window 96": ({"LSQ_WINDOW_ROWS": "96"}, dict(kind="csc", nwin=32, **_OFF))}
    for name, (env, expect) in forced.items():
        C.append(Config(name, "csc", (3000, 200), _FORCED, expect, "materialising" if name == "window 96" else "fused", env=env))
    for name in ("sliced 64 64", "sliced xmax 64"):
        env, expect = forced[name]
        C.append(Config(name + " nocolscale", "csc", (3000, 200), _FORCED, expect, "materialising", env=env, nocolscale=True))
    C += [
        Config("g:sliced", "csc", (140000, 64), _SLICED, _SLICED_EXPECT, "fused", model=True, fused=True),
        Config("g:sliced nocolscale", "csc", (140000, 64), _SLICED, _SLICED_EXPECT, None, model=True, nocolscale=True, lazy=True),
        Config("g:segments", "csc", (2500, 300), _SEGMENTS, dict(kind="csc", nwin=0, **_OFF), None, model=True),
        Config("g:windowed", "csc", (140000, 40), _WINDOWED, dict(kind="csc", windowed=True, **_OFF), None, model=True),
        Config("g:dense", "dense", (2100, 40), _cached(full_pattern, 2100, 40), dict(kind="dense"), None, model=True),
        Config("g:block", "block", (360, 45), _cached(block_pattern, 9, 40, 5), dict(kind="csc", **_OFF), None, model=True,
               block=(9, 40, 5)),
    ]
    return {c.name: c for c in C}


CONFIGS = _configs()


def layout_matches(lay, expect):
    """The subset of DeviceMatrix.layout() a configuration pins; returns the list of mismatches."""
    got = dict(kind=lay["kind"], srows=lay["srows"]["active"], scols=lay["scols"]["active"], ncw=lay["srows"]["ncw"],
               wrows=lay["srows"]["wrows"], ngw=lay["scols"]["ngw"], nwin=lay["nwin"], windowed=lay["nwin"] > 1)
    return [(k, got[k], v) for k, v in expect.items() if got[k] != v]


# ------------------------------------------------------------------------------------------------ the twin
def factors(rng, k):
    """k factors from [0.5, 0.8] or [1.25, 2]: never within 20 % of 1."""
    f = rng.uniform(1.25, 2.0, k)
    return np.where(rng.random(k) < 0.5, f, 1.0 / f)


def next_scale(s, rng):
    """For every entry of s (itself 1 or inside the two bands) a value inside the bands that also differs from it by a factor
    inside them, so that a cumulative multiplier never drifts and removing a scale later is a change of that size too.  The
    admissible set is up to four intervals (band of the value x band of the ratio); one is drawn by length, then a point."""
    lo = np.stack([np.maximum(a, r0 * s) for a, _ in ((0.5, 0.8), (1.25, 2.0)) for r0, _ in ((0.5, 0.8), (1.25, 2.0))])
    hi = np.stack([np.minimum(b, r1 * s) for _, b in ((0.5, 0.8), (1.25, 2.0)) for _, r1 in ((0.5, 0.8), (1.25, 2.0))])
    length = np.maximum(hi - lo, 0.0)
    assert np.all(length.sum(axis=0) > 0)
    cum = np.cumsum(length, axis=0)
    u = rng.random(s.size) * cum[-1]
    k = (u[None, :] >= cum).sum(axis=0)
    idx = np.arange(s.size)
    before = np.where(k > 0, cum[np.maximum(k - 1, 0), idx], 0.0)
    return np.clip(lo[k, idx] + (u - before), lo[k, idx], hi[k, idx])


def _segsum(v, ptr):
    out = np.zeros(len(ptr) - 1, dtype=v.dtype)
    ne = ptr[:-1] < ptr[1:]
    if v.size:
        out[ne] = np.add.reduceat(v, ptr[:-1][ne])
    return out


class Twin:
    """Stored values V (CSC order; dense: column-major; block / bordered: the handle's value order, which is CSC order of
    block_pattern), the scale s or None.  A model twin also keeps the model's A and the x of the latest g!."""

    def __init__(self, cfg, seed):
        self.cfg = cfg
        P = cfg.pattern
        self.m, self.n = P.shape
        self.indptr, self.indices = P.indptr.astype(np.int64), P.indices.astype(np.int64)
        self.cols = np.repeat(np.arange(self.n), np.diff(self.indptr))
        self.order = np.argsort(self.indices, kind="stable")          # CSC position of every entry in row-major order
        self.rptr = np.concatenate([[0], np.cumsum(np.bincount(self.indices, minlength=self.m))])
        self.Kcol, self.Krow = np.diff(self.indptr), np.diff(self.rptr)
        rng = np.random.default_rng(seed)
        self.V = rng.uniform(0.5, 1.5, self.indices.size) * rng.choice([-1.0, 1.0], self.indices.size)
        self.s = None
        self.cV = np.ones(self.V.size)
        self.A = self.V.copy() if cfg.model else None
        self.x_g = None
        if cfg.model and cfg.fused:
            self.s = np.ones(self.n)              # lsq_model_tanh_create installs the fused scale with s = 1
        # the readers' vectors: fixed for the configuration
        self.x, self.xadd = rng.standard_normal((2, self.n))
        self.y, self.yadd = rng.standard_normal((2, self.m))
        self.damp = rng.uniform(0.05, 1.05, self.n)
        self.empty_col = 1 if cfg.kind == "csc" else None
        if cfg.model:                             # the model's first g!: part of building the handle (its values are 0 before)
            self.mutate("g", rng)

    def copy(self):
        import copy
        t = copy.copy(self)
        t.V = self.V.copy()
        t.s = None if self.s is None else self.s.copy()
        return t

    @property
    def scaled(self):
        return self.s is not None

    # ---- mutations: each returns what the device side needs (new values, new scale, x of g!)
    def mutate(self, name, rng):
        if name in ("set_values", "async_wait", "async_nowait", "write_refresh", "fd"):
            c = next_scale(self.cV, rng)          # (the cumulative multiplier stays inside the bands: no drift of the scales)
            self.V, self.cV = self.V * (c / self.cV), c
            return self.V
        if name in ("set_colscale", "set_colscale_again", "s_inplace"):
            self.s = factors(rng, self.n) if self.s is None else next_scale(self.s, rng)
            return self.s
        if name in ("unscale", "unscale_plain"):
            self.s = None
            return None
        if name == "fd_refused":
            return None
        if name == "g":
            # 1 - tanh(x)^2 stays in [0.5, 0.8] (a factor of that size against the unscaled values) and moves by a factor from
            # the two bands against the previous one: down to [0.5, 0.8 p] (needs p >= 0.625) or up to [1.25 p, 0.8] (p <= 0.64)
            if self.x_g is None:
                new = rng.uniform(0.5, 0.8, self.n)
            else:
                p = 1.0 - np.tanh(self.x_g) ** 2
                up = (p < 0.625) | ((p <= 0.64) & (rng.random(self.n) < 0.5))
                u = rng.random(self.n)
                new = np.where(up, 1.25 * p + u * (0.8 - 1.25 * p), 0.5 + u * (0.8 * p - 0.5))
            self.x_g = np.arctanh(np.sqrt(1.0 - new)) * rng.choice([-1.0, 1.0], self.n)
            sfac = 1.0 - np.tanh(self.x_g) ** 2
            if self.cfg.fused:
                self.s = sfac                 # the model's g! IS lsq_mat_set_colscale(J, 1 - tanh(x)^2) on the stored values
            else:
                self.V, self.cV = self.A * sfac[self.cols], np.ones(self.V.size)
            return self.x_g
        raise KeyError(name)

    # ---- the effective matrix and the references
    def eff_ld(self):
        e = hp.ld(self.V)
        return e if self.s is None else e * hp.ld(self.s)[self.cols]

    def eff64(self):
        return self.V if self.s is None else self.V * self.s[self.cols]

    def scipy(self):
        return sp.csc_matrix((self.eff64(), self.indices, self.indptr), shape=(self.m, self.n))

    def product(self, trans, alpha, beta):
        """(ref, mag, K) of alpha J x + beta xadd-or-yadd in longdouble, per output element."""
        e = self.eff_ld()
        if not trans:
            t = (e * hp.ld(self.x)[self.cols])[self.order]
            dot, mag, add, K = _segsum(t, self.rptr), _segsum(np.abs(t), self.rptr), hp.ld(self.yadd), self.Krow
        else:
            t = e * hp.ld(self.y)[self.indices]
            dot, mag, add, K = _segsum(t, self.indptr), _segsum(np.abs(t), self.indptr), hp.ld(self.xadd), self.Kcol
        a, b = LD(alpha), LD(beta)
        return a * dot + b * add, abs(a) * mag + np.abs(b * add), K

    def sums(self, rows):
        e2 = self.eff_ld() ** 2
        return (_segsum(e2[self.order], self.rptr) if rows else _segsum(e2, self.indptr)).astype(np.float64)

    def stacked(self):
        A = self.scipy().toarray()
        return np.vstack([A, np.diag(np.sqrt(self.damp))]), np.concatenate([self.y, np.zeros(self.n)])

    def inv_gram(self):
        A = self.scipy().toarray()
        return np.linalg.inv(A.T @ A)


# ------------------------------------------------------------------------------------------------ sequences
def _seed(cfg, k):
    return 7919 * (1 + sorted(CONFIGS).index(cfg.name)) + 104729 * k


def sequences(cfg, count=None):
    """The committed sequences of a configuration: a list of lists of (mutation, readers).  Greedy: the next mutation is the
    legal one with the most uncovered (previous mutation, mutation) and (mutation, reader) pairs, ties by the seeded generator;
    the two readers are the least covered ones for that mutation.  The last step of a sequence runs every reader."""
    count = NSEQ[cfg.name] if count is None else count
    readers = cfg.readers
    seen_mm, seen_mr = set(), {}
    out = []
    for k in range(count):
        rng = np.random.default_rng(_seed(cfg, k))
        scaled, prev, steps = cfg.model and cfg.fused, None, []
        for step in range(SEQ_LEN):
            legal = [mu for mu in cfg.mutations if cfg.legal(mu, scaled)]
            # a new (previous, this) pair first, then the mutation from which most new pairs can start in the state it leaves,
            # then new readers
            def fresh_starts(mu):
                st = cfg.after(mu, scaled)
                return sum((mu, b) not in seen_mm for b in cfg.mutations if cfg.legal(b, st))
            score = [(prev is not None and (prev, mu) not in seen_mm) * 1000 + 10 * fresh_starts(mu)
                     + sum((mu, r) not in seen_mr for r in readers) + rng.random() for mu in legal]
            mu = legal[int(np.argmax(score))]
            if prev is not None:
                seen_mm.add((prev, mu))
            if step == SEQ_LEN - 1:
                rs = readers
            else:
                order = sorted(readers, key=lambda r: (seen_mr.get((mu, r), 0), rng.random()))
                rs = tuple(order[:2])
            for r in rs:
                seen_mr[mu, r] = seen_mr.get((mu, r), 0) + 1
            steps.append((mu, rs))
            scaled = cfg.after(mu, scaled)
            prev = mu
        out.append(steps)
    return out


def legal_pairs(cfg):
    """Every ordered (mutation, mutation) pair some state allows: the second must be legal in the state the first leaves."""
    pairs = set()
    for a in cfg.mutations:
        for state in (False, True):
            if state and cfg.model and not cfg.fused:     # no scale ever exists on a handle whose model multiplies out
                continue
            if cfg.legal(a, state):
                pairs.update((a, b) for b in cfg.mutations if cfg.legal(b, cfg.after(a, state)))
    return pairs


def coverage(cfg, seqs):
    mm, mr = set(), set()
    for steps in seqs:
        for i, (mu, rs) in enumerate(steps):
            mr.update((mu, r) for r in rs)
            if i:
                mm.add((steps[i - 1][0], mu))
    return mm, mr


def step_rng(cfg, k, step):
    return np.random.default_rng(_seed(cfg, k) + 31 * (step + 1))


# sequences per configuration: the smallest count at which the greedy walk covers every pair (asserted by the host file)
NSEQ = {"small": 10, "segments": 11, "windowed": 15, "rows-only": 7, "sliced": 11, "dense-small": 12, "dense": 11, "block": 12,
        "bordered": 13, "sliced 64 64": 10, "sliced xmax 64": 12, "window 96": 12, "sliced 64 64 nocolscale": 13,
        "sliced xmax 64 nocolscale": 11, "g:sliced": 5, "g:sliced nocolscale": 4, "g:segments": 4, "g:windowed": 4, "g:dense": 4,
        "g:block": 4}


# ------------------------------------------------------------------------------------------------ oracle 2
def fd_bound(twin, B, x):
    """|fd - B| per stored entry for the linear f(x) = B x: both evaluations carry the any-order dot-product error
    gamma_(K_i + 1) (|B| |x +- h e|)_i, their difference is divided by 2h (h = max(eps3 |x_j|, eps3), lsqhip.h), and the
    subtraction, the division and the forming of x +- h add three roundings of the quotient itself."""
    eps3 = float.fromhex("0x1.965fea53d6e41p-18")
    h = np.maximum(eps3 * np.abs(x), eps3)
    S = sp.csc_matrix((np.abs(B), twin.indices, twin.indptr), shape=(twin.m, twin.n))
    rowmag = S @ (np.abs(x) + h)
    g = np.asarray(ac.gamma(twin.Krow + 1), dtype=np.float64)
    return (2.0 * g[twin.indices] * rowmag[twin.indices]) / (2.0 * h[twin.cols]) + 8 * 2.0 ** -53 * np.abs(B) \
        + 2.0 * np.abs(B) * (2.0 ** -53 * (np.abs(x) + h) / h)[twin.cols]


def reference(twin, reader, oracle=None):
    """What judge() compares with; separated so that the host file can time and reuse it."""
    if reader == "values":
        return twin.V
    if reader in ("mul", "mul_t"):
        return [twin.product(reader == "mul_t", a, b) for a, b in ALPHA_BETA]
    if reader in ("colsum", "rowsum"):
        return twin.sums(reader == "rowsum")
    if reader == "ldiv:lsmr":
        J = oracle.Mat(dense=twin.scipy().toarray()) if twin.cfg.kind == "dense" else oracle.Mat.from_scipy(twin.scipy())
        st, xr, nmul, _ = oracle.ldiv(oracle.LSMR, J, twin.y, twin.damp)
        assert st == 0
        return xr, nmul
    if reader.startswith("ldiv:"):
        A, b = twin.stacked()
        return np.linalg.lstsq(A, b, rcond=None)[0]
    if reader == "gram":
        E = twin.scipy()
        return np.triu((E.T @ E).toarray()), np.triu((abs(E).T @ abs(E)).toarray())
    if reader in ("cov", "cov_qr"):
        return None if twin.empty_col is not None else twin.inv_gram()
    raise KeyError(reader)


def cov_pieces(twin, C):
    """The entries of inv(J'J) a covariance reader returns: (cov entries, stderr)."""
    cfg = twin.cfg
    se = np.sqrt(np.diag(C))
    if cfg.kind == "dense":
        return C.reshape(-1, order="F"), se
    B, mb, nb = cfg.block[:3]
    ng = cfg.block[3] if cfg.kind == "bordered" else 0
    loc = [C[b * nb:(b + 1) * nb, b * nb:(b + 1) * nb].reshape(-1) for b in range(B)]
    return np.concatenate(loc + ([C[B * nb:, B * nb:].reshape(-1)] if ng else [])), se


def judge(twin, reader, out, oracle=None, label=""):
    """Oracle 2: `out` (what read() returned on the device, or a planted host computation) against the twin.  Returns the
    worst ratio error / bound (<= 1 passes); asserts nothing, so that the host file can also demand a rejection."""
    ref = reference(twin, reader, oracle)
    if reader == "values":
        return 0.0 if np.array_equal(out[0], ref) else np.inf
    if reader in ("mul", "mul_t"):
        c = 4 if twin.scaled else 3
        return max(ac.product_excess(o, r, K, c, mag)[0] for o, (r, mag, K) in zip(out, ref))
    if reader in ("colsum", "rowsum"):
        d = np.abs(out[0] - ref)
        if np.any((ref == 0) & (d != 0)):
            return np.inf
        return float(np.max(np.where(ref == 0, 0.0, d / np.where(ref == 0, 1.0, 1e-13 * np.abs(ref)))))
    if reader == "ldiv:lsmr":
        xr, nmul = ref
        if int(out[1]) != nmul:
            return np.inf
        # test_column_scaled_jacobian's form of gpu_common's "rel 1e-8" for the fast kernels
        return float(np.max(np.abs(out[0] - xr)) / (1e-8 * max(1.0, np.max(np.abs(xr)))))
    if reader.startswith("ldiv:"):
        return float(np.max(np.abs(out[0] - ref)) / (1e-9 * np.max(np.abs(ref))))
    if reader == "gram":
        G, mag = ref
        bound = 2.0 * np.asarray(ac.gamma(twin.Kcol + 4), dtype=np.float64)[None, :] * mag
        d = np.abs(np.triu(out[0]) - G)
        if np.any((bound == 0) & (d != 0)):
            return np.inf
        return float(np.max(np.where(bound == 0, 0.0, d / np.where(bound == 0, 1.0, bound))))
    if reader in ("cov", "cov_qr"):
        if ref is None:          # the documented refusal: LSQ_ENOTPD at the (1-based) empty column
            return 0.0 if out == ("ENOTPD", twin.empty_col + 1) else np.inf
        cov, se = cov_pieces(twin, ref)
        return float(max(np.max(np.abs(out[0] - cov)) / (1e-9 * np.max(np.abs(cov))),
                         np.max(np.abs(out[1] - se)) / (1e-9 * np.max(se))))
    raise KeyError(reader)


def host_read(twin, reader, oracle=None):
    """A plain fp64 numpy evaluation of a reader on the twin: stands in for the device in the host file."""
    E = twin.scipy()
    if reader == "values":
        return (twin.V.copy(),)
    if reader == "mul":
        return tuple(a * (E @ twin.x) + b * twin.yadd for a, b in ALPHA_BETA)
    if reader == "mul_t":
        return tuple(a * (E.T @ twin.y) + b * twin.xadd for a, b in ALPHA_BETA)
    if reader in ("colsum", "rowsum"):
        return (np.asarray(E.multiply(E).sum(axis=1 if reader == "rowsum" else 0)).ravel(),)
    if reader == "ldiv:lsmr":
        return reference(twin, reader, oracle)            # (the CPU oracle's LSMR: x and the product count)
    if reader.startswith("ldiv:"):
        G = (E.T @ E).toarray() + np.diag(twin.damp)
        return (np.linalg.solve(G, E.T @ twin.y), 1)
    if reader == "gram":
        return (np.triu((E.T @ E).toarray()),)
    if reader in ("cov", "cov_qr"):
        if twin.empty_col is not None:
            return ("ENOTPD", twin.empty_col + 1)
        return cov_pieces(twin, twin.inv_gram())
    raise KeyError(reader)
