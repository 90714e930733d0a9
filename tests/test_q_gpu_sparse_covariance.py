"""Parameter covariance of a general sparse (CSC) Jacobian on the device: lsq_sparse_gram (k_sp_gram, lsq_cov_sparse.hip: the
dense G = J'J of the sparse handle, one wavefront and one LDS accumulator column per output column) and lsq_sparse_covariance
(that kernel, then the blocked Cholesky, explicit inverse, k_cov_xxt and k_cov_stderr of lsq_dense_covariance on an inner dense
solver).  Operands, twin and references: tests/sparse_cov_common.py, shown sound on the CPU by
tests/test_sparse_covariance_host.py.  Rule and metrics are the accuracy tier's, unchanged:
    Gram         every stored G_kj, k <= j, within ac.product_bound(K, c, mag) of its longdouble value; K = rows the two columns
                 share, c = further roundings read from the kernel: 0 (each term is a product and an add, which gamma_K covers),
                 2 on a column-scaled handle ((acc s_k) s_j, or the two factors rounded when the handle multiplies out), + 1
                 for the damping on the diagonal.  K = 0: exactly 0.
    covariance   ac.judge(ac.cov_pieces(.., k = n)): e_dev <= 16 max(e_ref, min(max(16, n), 64) 2^-53), H = hp.inv_gram(A) in
                 longdouble, e_ref numpy's fp64 inv(A.T @ A); covariance and stderr, with and without f.
"""
import ctypes as C
import time

import numpy as np
import pytest
import scipy.sparse as sp

import accuracy_common as ac
import fd_sparse_common as FS
import hp_reference as hp
import sparse_cov_common as sc
from gpu_common import lsq

pytestmark = pytest.mark.gpu

EARG, ENOTPD = lsq._lib.EARG, lsq._lib.ENOTPD
NAN = float("nan")


def lsmr_on(ctx, S):
    Jd = lsq.DeviceMatrix(ctx, S)
    return Jd, lsq.AllocatedSolver(Jd, lsq.LSMR(), for_lm=True)


def raw_gram(ctx, Jd, damp=None):
    """lsq_sparse_gram through the C ABI into an n x n buffer pre-filled with NaN: the whole buffer, column-major."""
    n = Jd.n
    dG = lsq.DeviceVector(ctx, n * n, np.full(n * n, NAN))
    dd = lsq.DeviceVector(ctx, n, damp) if damp is not None else None
    lsq._lib.check(lsq.lib().lsq_sparse_gram(Jd.h, dd.ptr if dd else None, dG.ptr))
    G = dG.get().reshape((n, n), order="F")
    dG.free()
    return G


def raw_cov(ctx, sv, Jd, f, want_cov, want_se):
    """lsq_sparse_covariance through the C ABI: (rc, cov or None, stderr or None, h_info)."""
    n = Jd.n
    dcov = lsq.DeviceVector(ctx, n * n) if want_cov else None
    dse = lsq.DeviceVector(ctx, n) if want_se else None
    df = lsq.DeviceVector(ctx, Jd.m, f) if f is not None else None
    info = np.full(1, -5, dtype=np.int32)
    rc = lsq.lib().lsq_sparse_covariance(sv.h, Jd.h, df.ptr if df else None, dcov.ptr if dcov else None,
                                         dse.ptr if dse else None, info.ctypes.data_as(lsq._lib.c_ip))
    return rc, (dcov.get() if want_cov and rc == 0 else None), (dse.get() if want_se and rc == 0 else None), int(info[0])


def judge_gram(label, G, S, colscale=None, damp=None, c=0):
    n = S.shape[1]
    assert np.all(np.isnan(G[np.tril_indices(n, -1)])), label + ": the strict lower triangle was written"
    U = np.triu(np.where(np.isnan(G), np.inf, G)) if n > 1 else G
    assert np.all(np.isfinite(U[np.triu_indices(n)])), label
    ref, mag, K = sc.gram_reference(S, colscale, damp)
    q, at = sc.gram_excess(U, ref, mag, K, c)
    print("ACC gram %s | %d x %d, nnz %d | worst |err| / bound %.3f at %s" % (label, S.shape[0], n, S.nnz, q, at))
    assert q <= 1.0, (label, q, at)


# ------------------------------------------------------------------------------------------ 1. the Gram kernel, per entry
def gram_patterns():
    rng = np.random.default_rng(11)
    full = sp.random(40, 200, density=0.03, format="lil", random_state=rng, data_rvs=rng.standard_normal)
    full[7, :] = rng.standard_normal(200)                          # four lane rounds
    long_col = sp.lil_matrix((3000, 6))                            # 64-entry batches with a ragged tail (3000 = 46 * 64 + 56)
    long_col[:, 2] = rng.standard_normal((3000, 1))
    for i, j in ((0, 0), (5, 1), (9, 1), (17, 3), (2999, 4), (1500, 5), (1501, 5)):
        long_col[i, j] = rng.standard_normal()
    return {"1x1": sp.csc_matrix(np.array([[1.7]])), "5x1": sp.csc_matrix(rng.standard_normal((5, 1))),
            "1x6": sp.csc_matrix(rng.standard_normal((1, 6))), "ragged300x65": ac.ragged_pattern(300, 65, 0.05, 3),
            "fullrow40x200": full.tocsc(), "longcol3000x6": long_col.tocsc()}


@pytest.mark.parametrize("name", list(gram_patterns()))
def test_gram_meets_the_product_bound(ctx, name):
    S = gram_patterns()[name]
    S.sort_indices()
    n = S.shape[1]
    Jd = lsq.DeviceMatrix(ctx, S)
    G = raw_gram(ctx, Jd)
    judge_gram(name, G, S)
    damp = 0.05 + np.random.default_rng(6).random(n)
    judge_gram(name + " damped", raw_gram(ctx, Jd, damp), S, damp=damp, c=1)
    # the Python entry: the same bits above the diagonal, zeros below
    P = lsq.sparse_gram(Jd)
    assert np.array_equal(P, np.triu(np.where(np.isnan(G), 0.0, G)))
    if name == "ragged300x65":
        assert np.all(G[:2, 1] == 0.0) and G[1, 1] == 0.0          # the empty column: exact zeros, diagonal included
    Jd.free()


@pytest.mark.parametrize("fused", [True, False])
def test_gram_column_scaled_handle(ctx, monkeypatch, fused):
    """V diag(s) with ac.product_scales: the sliced layouts and the fast kernels make lsq_mat_set_colscale take the fused mode
    (the stored values stay V, the kernel scales at its store); without them the handle multiplies out and the kernel reads J."""
    m, n = 300, 65
    V = ac.ragged_pattern(m, n, 0.05, 3)
    _, s = ac.product_scales(m, n, 5)
    if fused:
        monkeypatch.setenv("LSQ_SELL_FORCE", "1")
        lsq.set_exact(False)
    try:
        Jd = lsq.DeviceMatrix(ctx, V)
        ds = lsq.DeviceVector(ctx, n, s)
        Jd.set_colscale(ds)
        judge_gram("colscale %s" % ("fused" if fused else "multiplied out"), raw_gram(ctx, Jd), V, colscale=s, c=2)
        if fused:
            FS.same_bits(Jd.values(), V.data, "the stored values of a fused handle are V")
        Jd.free()
    finally:
        lsq.set_exact(None)


def test_gram_block_handles(ctx):
    bd = ac.bd_operand("plain", 5, 12, 4, 31).J                    # 60 x 20
    bb = ac.bb_operand("plain", 4, 10, 3, 5, 32).J                 # 40 x 17
    for label, J in (("block-diagonal handle", bd), ("bordered handle", bb)):
        Jd = lsq.DeviceMatrix(ctx, J)
        S = J.tocsc()
        S.sort_indices()
        G = raw_gram(ctx, Jd)
        judge_gram(label, G, S)
        Jd.free()


class RawHandle:
    """A CSC handle created through the C ABI from the arrays as given (DeviceMatrix goes through scipy, which sums repeated
    entries away)."""

    def __init__(self, ctx, m, n, colptr, rowval, vals):
        L = lsq.lib()
        self.ctx, self.m, self.n, self.sparse = ctx, m, n, True
        self.h = C.c_void_p()
        cp, rv = np.ascontiguousarray(colptr, dtype=np.int32), np.ascontiguousarray(rowval, dtype=np.int32)
        lsq._lib.check(L.lsq_csc_create(ctx.h, m, n, cp.ctypes.data_as(lsq._lib.c_ip), rv.ctypes.data_as(lsq._lib.c_ip), C.byref(self.h)))
        v = np.ascontiguousarray(vals, dtype=np.float64)
        lsq._lib.check(L.lsq_mat_set_values(self.h, v.ctypes.data_as(lsq._lib.c_dp)))

    def free(self):
        lsq.lib().lsq_mat_destroy(self.h)


def test_gram_repeated_entries(ctx):
    """A pattern that stores some (row, column) pairs more than once, which the products sum: in a short row (the 16-lane form)
    and in a row of 40 entries (the full-width form).  Small integers: exactly the Gram matrix of the summed pattern."""
    m, n = 6, 40
    rng = np.random.default_rng(8)
    trip = [(0, j) for j in range(n)] + [(0, 3), (0, 3), (0, 39)]            # the long row, column 3 three times, 39 twice
    trip += [(2, 3), (2, 3), (2, 5), (4, 5), (4, 5), (4, 5), (4, 39), (5, 0), (5, 0)]
    trip.sort(key=lambda t: (t[1], t[0]))
    rows, cols = np.array([t[0] for t in trip]), np.array([t[1] for t in trip])
    vals = rng.integers(1, 6, len(trip)).astype(float)
    colptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=n))])
    S = sp.coo_matrix((vals, (rows, cols)), shape=(m, n)).tocsc()            # (sums the repeated pairs)
    assert S.nnz < len(trip)
    Jd = RawHandle(ctx, m, n, colptr, rows, vals)
    G = raw_gram(ctx, Jd)
    assert np.all(np.isnan(G[np.tril_indices(n, -1)]))
    assert np.array_equal(np.triu(np.where(np.isnan(G), 0.0, G)), np.triu((S.T @ S).toarray()))
    Jd.free()


# ------------------------------------------------------------------------------------------ 2. geometry, exact arithmetic
def device_columns(ctx, dG, n, cols):
    """Columns of the n x n device buffer, and its diagonal, copied out by offset."""
    L = lsq.lib()
    base = dG.ptr.value
    out = {}
    for j in cols:
        col = np.empty(n)
        lsq._lib.check(L.lsq_d2h(ctx.h, col.ctypes.data_as(C.c_void_p), C.c_void_p(base + 8 * j * n), 8 * n))
        out[j] = col
    return out


def device_diagonal(ctx, dG, n):
    L = lsq.lib()
    base = dG.ptr.value
    d = np.empty(n)
    for j in range(n):
        lsq._lib.check(L.lsq_d2h(ctx.h, C.c_void_p(d.ctypes.data + 8 * j), C.c_void_p(base + 8 * j * (n + 1)), 8))
    return d


GEOMETRY_NS = [n for pair in sc.W_SWITCHES for n in pair] + [sc.GRAM_MAX_N]


@pytest.mark.parametrize("n", GEOMETRY_NS)
def test_geometry_switches_exact(ctx, n):
    """A band of small integers (at most three entries per row: every sum is exact) at the n on either side of each change of
    W -- 5120 | 5121 (4 -> 3 wavefronts per workgroup), 6826 | 6827 (3 -> 2), 10240 | 10241 (2 -> 1) -- and at the limit 16384.
    Up to n = 5121 the whole matrix is downloaded and compared; beyond (the download and the dense scipy product then take
    more than 5 s: 0.4 to 2.1 GB) the whole diagonal and columns 0, 1, 2, n - 3, n - 2, n - 1 and 58 seeded others, whole from
    row 0 to the diagonal, are copied out by offset and compared, and the strict lower part of each of these columns must
    still hold the NaN the buffer was filled with."""
    m = n + 2
    S = sc.band_int(m, n, n)
    assert sc.gram_waves(n) == {5120: 4, 5121: 3, 6826: 3, 6827: 2, 10240: 2, 10241: 1, 16384: 1}[n]
    Jd = lsq.DeviceMatrix(ctx, S)
    ref = sp.triu(S.T @ S).tocsc()
    t0 = time.time()
    if n <= 5121:
        G = raw_gram(ctx, Jd)
        assert np.all(np.isnan(G[np.tril_indices(n, -1)]))
        assert np.array_equal(np.triu(np.where(np.isnan(G), 0.0, G)), ref.toarray())
    else:
        L = lsq.lib()
        p = C.c_void_p()
        lsq._lib.check(L.lsq_malloc(ctx.h, 8 * n * n, C.byref(p)))
        dG = lsq.DeviceVector.borrow(ctx, n * n, p)
        try:
            lsq._lib.check(L.lsq_fill(ctx.h, n * n, NAN, p))
            lsq._lib.check(L.lsq_sparse_gram(Jd.h, None, p))
            rng = np.random.default_rng(n)
            cols = sorted(set([0, 1, 2, n - 3, n - 2, n - 1]) | set(int(c) for c in rng.choice(n, 58, replace=False)))
            got = device_columns(ctx, dG, n, cols)
            for j in cols:
                want = ref[:, [j]].toarray().reshape(-1)
                assert np.array_equal(got[j][:j + 1], want[:j + 1]), j
                assert np.all(np.isnan(got[j][j + 1:])), j
            assert np.array_equal(device_diagonal(ctx, dG, n), ref.diagonal())
        finally:
            L.lsq_free(ctx.h, p)
    print("geometry n = %d: W = %d, %.2f s" % (n, sc.gram_waves(n), time.time() - t0))
    Jd.free()


def test_above_the_limit_is_refused(ctx):
    n = sc.GRAM_MAX_N + 1
    S = sc.band_int(n + 2, n, 1)
    Jd, sv = lsmr_on(ctx, S)
    L = lsq.lib()
    out = lsq.DeviceVector(ctx, 16)
    for entry, call in (("lsq_sparse_gram", lambda: L.lsq_sparse_gram(Jd.h, None, out.ptr)),
                        ("lsq_sparse_covariance", lambda: L.lsq_sparse_covariance(sv.h, Jd.h, None, None, out.ptr, None))):
        rc = call()
        msg = L.lsq_last_error().decode()
        assert rc == EARG and msg.startswith(entry + ": n = %d is above the limit of %d columns" % (n, sc.GRAM_MAX_N)), (rc, msg)
    with pytest.raises(lsq.ArgumentError):
        sv.sparse_covariance(cov=False)
    sv.free()
    Jd.free()


# ------------------------------------------------------------------------------------------ 3. accuracy of the covariance
def blocked_shape(m, n):
    return n >= 32 or (n >= 2 and m * n >= 20000)                  # lsq_cholesky_takes_blocked


@pytest.mark.parametrize("m,n,family", sc.CASES)
def test_accuracy(ctx, m, n, family):
    op, r = sc.case(family, m, n)
    Jd, sv = lsmr_on(ctx, op.S)
    pieces = []
    for with_f in (False, True):
        cov = sv.sparse_covariance(f=op.f if with_f else None)
        assert cov.n == n and cov.cov.shape == (n, n) and cov.stderr.shape == (n,)
        pieces += r.pieces("f" if with_f else "unscaled", cov.cov, cov.stderr, with_f)
        print("PATH sparse covariance %dx%d %s | %s" % (m, n, family, cov.chol_path))
        assert cov.chol_path in (("blocked", "blocked-one-launch") if blocked_shape(m, n) else ("one-workgroup",))
        assert sv.info()["chol_path"] == cov.chol_path
    ac.judge("sparse covariance %s %dx%d" % (family, m, n), pieces)
    sv.free()
    Jd.free()


@pytest.mark.parametrize("m,n", [(90, 31), (300, 65)])
def test_accuracy_column_scaled_handle(ctx, m, n):
    """graded as a column-scaled handle: V plain, s the grading; the reference is V diag(s) formed in longdouble."""
    op, _ = sc.case("graded", m, n)
    r = sc.Ref(op.S.toarray(), op.f, A_hp=hp.ld(op.V.toarray()) * hp.ld(op.s))
    Jd = lsq.DeviceMatrix(ctx, op.V)
    ds = lsq.DeviceVector(ctx, n, op.s)
    Jd.set_colscale(ds)
    cov = lsq.sparse_covariance(Jd, f=op.f)
    ac.judge("sparse covariance colscale %dx%d" % (m, n), r.pieces("f", cov.cov, cov.stderr, True))
    Jd.free()


# ------------------------------------------------------------------------------------------ 4. beyond one CU's worth of tiles
def block_case(B):
    S, blocks = sc.block_pattern(B, 12, 8, 40 + B)
    f = np.random.default_rng(B).standard_normal(S.shape[0])
    return S, blocks, f


def judge_blocks(label, cov, blocks, f, nb=8):
    n = cov.n
    m = sum(b.shape[0] for b in blocks)
    s2_hp, s2 = ac.s2_of(f, m - n), float(f @ f) / (m - n)
    mask = np.kron(np.eye(len(blocks), dtype=bool), np.ones((nb, nb), dtype=bool))
    assert np.count_nonzero(cov.cov[~mask]) == 0, label + ": an entry outside the blocks is not +-0"
    pieces = []
    for b, A in enumerate(blocks):
        sl = slice(b * nb, (b + 1) * nb)
        pieces += ac.cov_pieces("block %d" % b, cov.cov[sl, sl], cov.stderr[sl], s2 * np.linalg.inv(A.T @ A), hp.inv_gram(A) * s2_hp, nb)
    ac.judge(label, pieces)


def test_block_pattern_beyond_one_launch(ctx):
    """641 blocks of 8 columns on a PLAIN CSC handle: n = 5128, past the one-launch factorisation (3321 tiles) and past the
    first change of W; every diagonal 8 x 8 block against its own longdouble inverse, everything else exactly +-0."""
    S, blocks, f = block_case(641)
    assert S.shape[1] == 5128 and sc.gram_waves(5128) == 3
    Jd, sv = lsmr_on(ctx, S)
    t0 = time.time()
    cov = sv.sparse_covariance(f=f)
    print("n = 5128: %.2f s, %s" % (time.time() - t0, cov.chol_path))
    assert cov.chol_path == "blocked"
    assert np.array_equal(cov.cov, cov.cov.T)
    judge_blocks("sparse covariance 641 blocks of 8", cov, blocks, f)
    sv.free()
    Jd.free()


@pytest.mark.parametrize("env,expect", [({}, "blocked-one-launch"), ({"LSQ_CHOL_PANELS": "1"}, "blocked")])
def test_both_factorisations(ctx, monkeypatch, env, expect):
    S, blocks, f = block_case(40)                                  # n = 320: 15 tiles, which the one-launch factorisation accepts
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    Jd, sv = lsmr_on(ctx, S)
    cov = sv.sparse_covariance(f=f)
    assert cov.chol_path == expect
    judge_blocks("sparse covariance 40 blocks of 8, %s" % expect, cov, blocks, f)
    sv.free()
    Jd.free()


def test_one_launch_gives_up_and_panels_take_over(ctx, monkeypatch):
    S, blocks, f = block_case(40)
    Jd, sv = lsmr_on(ctx, S)
    clean = sv.sparse_covariance(f=f)
    before = sv.stats()["chol_one_launch"]["giveups"]
    monkeypatch.setenv("LSQ_TEST_EXCHANGE_TIMEOUT", "1")
    cov = sv.sparse_covariance(f=f)
    monkeypatch.delenv("LSQ_TEST_EXCHANGE_TIMEOUT")
    assert sv.stats()["chol_one_launch"]["giveups"] == before + 1
    assert clean.chol_path == "blocked-one-launch" and cov.chol_path == "blocked"
    judge_blocks("sparse covariance after a give-up", cov, blocks, f)     # (the Gram kernel ran again: d_chol held the wreck)
    sv.free()
    Jd.free()


# ------------------------------------------------------------------------------------------ 5. bits
@pytest.mark.parametrize("m,n", [(50, 3), (300, 65), (500, 130)])
def test_bits(ctx, m, n):
    op, _ = sc.case("plain", m, n)
    Jd, sv = lsmr_on(ctx, op.S)

    def run():
        return raw_gram(ctx, Jd), sv.sparse_covariance(f=op.f)

    G, a = run()
    assert np.all(np.isfinite(a.cov)) and np.all(np.isfinite(a.stderr))
    assert np.array_equal(a.cov, a.cov.T)
    G2, b = run()
    lsq.debug_set(serial=1)
    try:
        G3, ser = run()
    finally:
        lsq.debug_set(serial=0)
    lsq.debug_set(launch_jitter_us=200)
    try:
        G4, jit = run()
    finally:
        lsq.debug_set(launch_jitter_us=0)
    for label, (Gx, x) in (("again", (G2, b)), ("serial", (G3, ser)), ("jitter", (G4, jit))):
        FS.same_bits(Gx, G, label + " G")
        FS.same_bits(x.cov, a.cov, label + " cov")
        FS.same_bits(x.stderr, a.stderr, label + " stderr")
    # stderr: the same bits with and without d_cov; and sqrt(diag(cov)) to rounding (tests/test_j_gpu_dense_covariance.py)
    rc1, cov1, se1, _ = raw_cov(ctx, sv, Jd, op.f, True, True)
    rc2, none2, se2, _ = raw_cov(ctx, sv, Jd, op.f, False, True)
    rc3, cov3, _, _ = raw_cov(ctx, sv, Jd, op.f, True, False)
    assert (rc1, rc2, rc3) == (0, 0, 0) and none2 is None
    assert np.array_equal(se1, se2) and np.array_equal(se1, a.stderr)
    assert np.array_equal(cov1, cov3) and np.array_equal(cov1.reshape((n, n), order="F"), a.cov)
    assert np.all(np.abs(se1 - np.sqrt(np.diag(a.cov))) <= (2 * n + 8) * ac.UNIT * se1)
    # a fresh solver, and the module-level entry: the same bits
    fresh = lsq.sparse_covariance(Jd, f=op.f)
    FS.same_bits(fresh.cov, a.cov)
    FS.same_bits(fresh.stderr, a.stderr)
    sv.free()
    Jd.free()


# ------------------------------------------------------------------------------------------ 6. against what exists
def test_block_diagonal_handle_against_solver_covariance(ctx):
    B, mb, nb = 6, 20, 5
    op = ac.bd_operand("plain", B, mb, nb, 51)
    Jd = lsq.DeviceMatrix(ctx, op.J)
    old = lsq.covariance(Jd)                                        # lsq_solver_covariance, unscaled
    new = lsq.sparse_covariance(Jd)
    n = B * nb
    mask = np.kron(np.eye(B, dtype=bool), np.ones((nb, nb), dtype=bool))
    assert np.count_nonzero(new.cov[~mask]) == 0
    pieces = []
    for b in range(B):
        A = op.J.block(b)
        H, R = hp.inv_gram(A), np.linalg.inv(A.T @ A)
        sl = slice(b * nb, (b + 1) * nb)
        pieces += ac.cov_pieces("new block %d" % b, new.cov[sl, sl], new.stderr[sl], R, H, nb)
        pieces += ac.cov_pieces("old block %d" % b, old.block(b), old.stderr[sl], R, H, nb)
    ac.judge("block-diagonal handle, both entries", pieces)
    assert n == new.n
    Jd.free()


def test_bordered_handle_against_solver_covariance_and_cross_blocks(ctx):
    B, mb, nb, ng = 4, 14, 4, 3
    op = ac.bb_operand("plain", B, mb, nb, ng, 52)
    J = op.J
    m, n = J.shape
    Jd = lsq.DeviceMatrix(ctx, J)
    old = lsq.covariance(Jd, f=op.y)
    new = lsq.sparse_covariance(Jd, f=op.y)
    A = J.toarray()
    s2_hp, s2 = ac.s2_of(op.y, m - n), float(op.y @ op.y) / (m - n)
    H = hp.inv_gram(A) * s2_hp                                     # the whole n x n inverse, cross blocks included
    R = np.linalg.inv(A.T @ A) * s2
    locals_hp, shared_hp = hp.inv_gram(J)
    g = slice(B * nb, n)
    assert float(np.max(np.abs(H[g, g] - shared_hp * s2_hp) / np.abs(H[g, g]))) < 1e-15      # (the two longdouble routes agree)
    pieces = ac.cov_pieces("new, whole matrix", new.cov, new.stderr, R, H, n)
    for b in range(B):
        sl = slice(b * nb, (b + 1) * nb)
        pieces += ac.cov_pieces("new block %d" % b, new.cov[sl, sl], new.stderr[sl], R[sl, sl], H[sl, sl], nb)
        pieces += ac.cov_pieces("old block %d" % b, old.block(b), old.stderr[sl], R[sl, sl], H[sl, sl], nb)
        # the cross-covariance -W_b Cov_gg, which lsq_solver_covariance does not form: by the metric, against H
        sd = np.sqrt(np.diag(H))
        e_new = float(np.max(np.abs(hp.ld(new.cov[sl, g]) - H[sl, g]) / np.outer(sd[sl], sd[g])))
        e_ref = float(np.max(np.abs(hp.ld(R[sl, g]) - H[sl, g]) / np.outer(sd[sl], sd[g])))
        pieces.append(("new cross block %d" % b, e_new, e_ref, nb + ng))
        assert np.array_equal(new.cov[sl, g], new.cov[g, sl].T)
    pieces += ac.cov_pieces("new shared", new.cov[g, g], new.stderr[g], R[g, g], H[g, g], ng)
    pieces += ac.cov_pieces("old shared", old.shared, old.stderr[g], R[g, g], H[g, g], ng)
    ac.judge("bordered handle, both entries", pieces)
    Jd.free()


# ------------------------------------------------------------------------------------------ 7. failure and refusals
def test_empty_column_then_reuse(ctx):
    m, n, zc = 400, 70, 66                                         # (column 66: inside the second 64-block)
    good = sc.pattern(m, n, 5)
    bad = good.tolil()
    bad[:, zc] = 0
    bad = bad.tocsc()
    bad.eliminate_zeros()
    assert bad.indptr[zc] == bad.indptr[zc + 1]                    # structurally empty
    msg = "PosDefException: matrix is not positive definite; Cholesky failed at %d" % (zc + 1)
    Jb, sb = lsmr_on(ctx, bad)
    rc, _, _, info = raw_cov(ctx, sb, Jb, None, True, True)
    assert rc == ENOTPD and info == zc + 1
    assert lsq.lib().lsq_last_error().decode() == msg
    with pytest.raises(lsq.PosDefException) as ec:
        sb.sparse_covariance()
    assert ec.value.status == ENOTPD and str(ec.value) == msg
    # the same solver on a good operand of the same shape: the bits of a fresh solver (nothing stale is read)
    f = np.random.default_rng(5).standard_normal(m)
    Jg = lsq.DeviceMatrix(ctx, good)
    again = lsq.DenseCovariance(n, *raw_cov(ctx, sb, Jg, f, True, True)[1:3])
    fresh = lsq.sparse_covariance(Jg, f=f)
    assert np.all(np.isfinite(again.cov)) and np.all(np.isfinite(again.stderr))
    FS.same_bits(again.cov, fresh.cov)
    FS.same_bits(again.stderr, fresh.stderr)
    # ... and it still solves (its own handle: the operand with the empty column, damped)
    x = lsq.DeviceVector(ctx, n)
    sb.ldiv_(x, lsq.DeviceVector(ctx, m, f), lsq.DeviceVector(ctx, n, np.full(n, 0.1)))
    D, xs = bad.toarray(), x.get()
    assert xs[zc] == 0.0 and np.all(np.isfinite(xs))
    assert np.sum((D @ xs - f) ** 2) + 0.1 * np.sum(xs ** 2) < np.sum(f ** 2)      # (x = 0 gives |f|^2)
    for o in (sb, Jb, Jg):
        o.free()


def test_refusals(ctx):
    L = lsq.lib()
    m, n = 12, 3
    rng = np.random.default_rng(3)
    A = rng.standard_normal((m, n))
    csc, lsmr = lsmr_on(ctx, sp.csc_matrix(A))
    out = lsq.DeviceVector(ctx, 64)
    f = lsq.DeviceVector(ctx, 64)
    dense = lsq.DeviceMatrix(ctx, A)
    op = lsq.DeviceOperator(ctx, m, n, lambda trans, x, o: None, lambda o: None)
    bd = lsq.DeviceMatrix(ctx, lsq.BlockDiagonal(4, 3, 3, data=lsq.synthetic.blockdiag_inputs(4, 3, 3, 1)))      # 12 x 12
    other = lsq.DeviceMatrix(ctx, sp.csc_matrix(rng.standard_normal((m, n + 1))))
    square, lsmr_sq = lsmr_on(ctx, sp.csc_matrix(rng.standard_normal((n, n)) + 3 * np.eye(n)))
    wide, lsmr_wide = lsmr_on(ctx, sp.csc_matrix(rng.standard_normal((2, n))))
    hooked = lsq.AllocatedSolver(csc, lsq.LSMR(), for_lm=True)
    hook = lsq._lib.ROW_ALLREDUCE_CALLBACK(lambda buf, count, stream, user: 0)
    lsq._lib.check(L.lsq_solver_set_row_allreduce(hooked.h, hook, None, 4 * m))
    cases = [
        ("both outputs NULL", lsmr, csc, None, None, None, "d_cov and d_stderr are both NULL"),
        ("a dense handle", lsmr, dense, None, out.ptr, None, "lsq_dense_covariance"),
        ("an operator handle", lsmr, op, None, out.ptr, None, "operator handle"),
        ("a Cholesky solver on a block-diagonal handle", lsq.AllocatedSolver(bd, lsq.Cholesky(), for_lm=True), bd, None, None,
         out.ptr, "needs the LSMR() solver"),
        ("a solver of another shape", lsmr, other, None, out.ptr, None, "was allocated for a 12 x 3 Jacobian, got 12 x 4"),
        ("a row all-reduce hook", hooked, csc, None, out.ptr, None, "row all-reduce hook"),
        ("m = n with f", lsmr_sq, square, f.ptr, out.ptr, out.ptr, "needs m > n"),
        ("m < n with f", lsmr_wide, wide, f.ptr, None, out.ptr, "needs m > n"),
    ]
    for label, sv, J, pf, pcov, pse, needle in cases:
        rc = L.lsq_sparse_covariance(sv.h, J.h, pf, pcov, pse, None)
        msg = L.lsq_last_error().decode()
        print(label, "->", rc, msg)
        assert rc == EARG, (label, rc)
        assert msg.startswith("lsq_sparse_covariance:") and needle in msg, (label, msg)
    for label, J, needle in (("a dense handle", dense, "dense handle"), ("an operator handle", op, "operator handle")):
        rc = L.lsq_sparse_gram(J.h, None, out.ptr)
        msg = L.lsq_last_error().decode()
        assert rc == EARG and msg.startswith("lsq_sparse_gram:") and needle in msg, (label, rc, msg)
    with pytest.raises(lsq.ArgumentError):
        lsq.sparse_covariance(dense)
    with pytest.raises(lsq.ArgumentError):
        lsq.sparse_gram(dense)
    # lsq_dense_covariance still refuses the CSC handle with its own message; n = 0 is served and launches nothing
    chol = lsq.AllocatedSolver(dense, lsq.Cholesky(), for_lm=True)
    assert L.lsq_dense_covariance(chol.h, csc.h, None, out.ptr, None, None) == EARG
    assert "CSC and operator handles are not offered" in L.lsq_last_error().decode()
    empty, lsmr_e = lsmr_on(ctx, sp.csc_matrix((5, 0)))
    assert L.lsq_sparse_covariance(lsmr_e.h, empty.h, None, out.ptr, out.ptr, None) == 0
    assert L.lsq_sparse_gram(empty.h, None, out.ptr) == 0
    # the solver still works after the refusals; m = n without f is served; cov=False returns the standard errors only
    cov = lsmr.sparse_covariance()
    H = hp.inv_gram(A)
    ac.judge("sparse covariance after refusals", ac.cov_pieces("unscaled", cov.cov, cov.stderr, np.linalg.inv(A.T @ A), H, n))
    assert np.all(np.isfinite(lsmr_sq.sparse_covariance().cov))
    se = lsmr.sparse_covariance(cov=False)
    assert se.cov is None and np.array_equal(se.stderr, cov.stderr) and se.chol_path == cov.chol_path
    assert set(lsmr.info()) == set(chol.info())                    # no new keys


# ------------------------------------------------------------------------------------------ 8. after a fit
def test_standard_errors_after_a_sparse_fit(ctx):
    """r = A tanh(x) - y on a 61 x 23 random pattern with 1 % noise, LevenbergMarquardt(LSMR()) on the device's coloured
    central differences; then the Jacobian at the solution by the same differences, lsq_sparse_covariance with the residual
    there, and the standard errors by the rule against numpy on the downloaded Jacobian."""
    S = FS.random_pattern(11, 61, 23, 0.2)
    f_, _, x0, x_true = FS.tanh_fit_problem(S, 5)
    m, n = S.shape
    nls = lsq.LeastSquaresProblem(x=x0.copy(), y=np.zeros(m), f_=f_, J=S.copy(), autodiff="central_coloured")
    r = lsq.optimize_(nls, lsq.LevenbergMarquardt(lsq.LSMR()), iterations=60, ctx=ctx)
    assert r.converged
    x = np.array(r.minimizer)
    Jd = lsq.DeviceMatrix(ctx, S)
    Jd.set_fd_colouring(None)
    lsq.fd_jacobian_(Jd, x, f_)
    fcur = np.zeros(m)
    f_(fcur, x)
    sv = lsq.AllocatedSolver(Jd, lsq.LSMR(), for_lm=True)
    cov = sv.sparse_covariance(f=fcur)
    A = sp.csc_matrix((Jd.values(), S.indices, S.indptr), shape=S.shape).toarray()
    ref = sc.Ref(A, fcur)
    print("fit: %d iterations, ssr %.3e, max stderr %.3e, %s" % (r.iterations, r.ssr, np.max(cov.stderr), cov.chol_path))
    ac.judge("sparse covariance after a fit", ref.pieces("f", cov.cov, cov.stderr, True))
    assert np.all(np.abs(x - x_true) <= 8 * cov.stderr + 1e-3)      # the errors ARE of the size the noise leaves
    sv.free()
    Jd.free()
