"""Accuracy tier on the device, products: J x and J'y on every layout the shape tier forces, judged PER OUTPUT ELEMENT.

tests/test_b_gpu_kernels.py bounds |out - ref| by 1e-12 (1 + max row abs sum): one scale for the whole vector, so a row or a
column a few decades below the largest is not checked at all.  Here every output must satisfy the standard dot-product bound,
valid for any summation order with or without FMA,

    |out_i - ref_i| <= gamma_(K_i + c) (|alpha| sum_k |a_ik x_k| + |beta y_i|),   gamma_t = t u / (1 - t u),  u = 2^-53

(ac.product_bound; ref_i and the right-hand side formed in longdouble from dense copies).  K_i: the stored entries that
contribute to output i.  c, counted from the kernels: the epilogue of every product is `alpha * dot + beta * y`
(EpiAxpby::seg in lsq_sparse.hip, lsq_dense.hip, lsq_exact.hip): alpha * dot, beta * y and the add are three roundings, c = 3;
partial sums of windows, slices and wavefronts are added in some order, which the any-order bound of K_i terms already covers.
A column-scaled handle adds ONE rounding per entry: fused (sliced layouts) J x gathers fl(s_k x_k) and J'y scales the combined
dot by s_j; elsewhere the handle stores fl(v_ik s_k).  c = 4 there.

Operand: diag(r) S diag(c), S the ragged pattern of test_sparse_products (an empty row, an empty column, one full row), r and
c spread over 12 decades each and shuffled, so that neighbours in a slice, a window or a wavefront differ in scale: an output
of size 1e-12 sits beside one of size 1.  The vectors are balanced against the scales (ac.product_vectors: x = z / c, the
addend y = r z'), so that every stored entry matters to its output and the beta term hides none.  tests/test_accuracy_host.py shows that the bound accepts numpy's own product in
reversed and pairwise order and rejects a float32 x and one dropped entry of the smallest row."""
import functools

import numpy as np
import pytest

import accuracy_common as ac
import hp_reference as hp
from gpu_common import lsq

pytestmark = pytest.mark.gpu

SHAPES = [(3000, 200, 0.01), (500, 40, 0.5), (64, 3000, 0.02)]
PLANS = ("LSQ_PLAN_CSC", "LSQ_PLAN_CSR")


def plan_env(plan, window=None):
    env = {k: plan for k in PLANS}
    if window:
        env["LSQ_WINDOW_ROWS"] = str(window)
    return env


LAYOUTS = {"default": {}}
for _plan in ("stream", "wave", "block"):
    LAYOUTS[_plan] = plan_env(_plan)
    LAYOUTS[_plan + " window 96"] = plan_env(_plan, 96)
LAYOUTS.update({"window 96": {"LSQ_WINDOW_ROWS": "96"},
                "sliced": {"LSQ_SELL_FORCE": "1"},
                "sliced 64 64": {"LSQ_SELL_FORCE": "1", "LSQ_SELL_ROWS": "64", "LSQ_SELL_GROWS": "64"},
                "sliced xmax 64": {"LSQ_SELL_FORCE": "1", "LSQ_SELL_XMAX": "64"}})


def assert_layout(lay, layout, m, n, nnz, scaled):
    """DeviceMatrix.layout() says what the switches of LAYOUTS[layout] were to build (lsq_csc_create): the plans as named; the
    CSC windows of LSQ_WINDOW_ROWS where m exceeds a window; the sliced columns under LSQ_SELL_FORCE, and the sliced rows where
    the rows keep the stream plan (fewer than 48 entries per row on average: not 64 x 3000) and x needs at most 32 column
    windows; the fused column scale exactly where both sliced layouts exist."""
    env = LAYOUTS[layout]
    assert lay["kind"] == "csc"
    for key, plan in (("csr_plan", env.get("LSQ_PLAN_CSR")), ("csc_plan", env.get("LSQ_PLAN_CSC"))):
        assert plan is None or lay[key] == plan, (layout, lay)
    rw = int(env.get("LSQ_WINDOW_ROWS", 0))
    assert lay["nwin"] == (-(-m // rw) if rw and m > rw else 0), (layout, lay)
    forced = "LSQ_SELL_FORCE" in env
    ncw = -(-n // int(env["LSQ_SELL_XMAX"])) if "LSQ_SELL_XMAX" in env else 1
    rows = forced and nnz / m < 48 and ncw <= 32
    assert lay["scols"]["active"] == forced and lay["srows"]["active"] == rows, (layout, lay)
    if rows:
        assert lay["srows"]["ncw"] == ncw, (layout, lay)
        if "LSQ_SELL_ROWS" in env:
            assert lay["srows"]["wrows"] == int(env["LSQ_SELL_ROWS"]), (layout, lay)
    if forced and "LSQ_SELL_GROWS" in env:
        assert lay["scols"]["ngw"] == -(-m // int(env["LSQ_SELL_GROWS"])), (layout, lay)
    assert lay["colscale"] == ((("fused" if rows else "materialising")) if scaled else None), (layout, lay)


class ProductRef:
    """The operand as the plain handle stores it (fl(r_i s_ik c_k)) and as the column-scaled handle means it (fl(r_i s_ik) c_k,
    unrounded), x, y, and per (scaled handle, trans) the longdouble reference, the magnitude and the entry counts."""

    def __init__(self, A_plain, V, r, s, seed):
        self.m, self.n = A_plain.shape
        self.fwd, self.adj = ac.product_vectors(r, s, seed)          # (x, y) of J x; (y, x) of J'y
        self.eff = {False: hp.ld(A_plain), True: hp.ld(V) * hp.ld(s)}
        self.K = {False: np.count_nonzero(A_plain, axis=1), True: np.count_nonzero(A_plain, axis=0)}
        self._ref = {}

    def ref(self, scaled, trans):
        if (scaled, trans) not in self._ref:
            A = self.eff[scaled]
            self._ref[scaled, trans] = (ac.product_reference(A.T, self.adj[0], -2.0, 0.25, self.adj[1]) if trans else
                                        ac.product_reference(A, self.fwd[0], 1.5, -0.5, self.fwd[1]))
        return self._ref[scaled, trans]


@functools.lru_cache(maxsize=2)
def sparse_case(m, n, density):
    S = ac.ragged_pattern(m, n, density, m + n)
    r, c = ac.product_scales(m, n, m + 2 * n)
    V = (S.multiply(r[:, None])).tocsc()                  # diag(r) S
    P = (V.multiply(c[None, :])).tocsc()                  # fl(diag(r) S diag(c)): what the plain handle stores
    for M in (V, P):
        M.sort_indices()
    assert np.array_equal(V.indices, P.indices) and np.all(P.data != 0) and np.all(np.isfinite(P.data))
    return V, P, c, ProductRef(P.toarray(), V.toarray(), r, c, m * n)


def judge_both_products(ctx, J, ref, scaled, label):
    m, n = ref.m, ref.n
    c = 4 if scaled else 3
    out = lsq.mul_(lsq.DeviceVector(ctx, m, ref.fwd[1]), J, lsq.DeviceVector(ctx, n, ref.fwd[0]), 1.5, -0.5).get()
    val, mag = ref.ref(scaled, False)
    ac.judge_product(label + " J x", out, val, ref.K[False], c, mag)
    out = lsq.mul_(lsq.DeviceVector(ctx, n, ref.adj[1]), J, lsq.DeviceVector(ctx, m, ref.adj[0]), -2.0, 0.25, trans=True).get()
    val, mag = ref.ref(scaled, True)
    ac.judge_product(label + " J'y", out, val, ref.K[True], c, mag)


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("m,n,density", SHAPES)
def test_sparse_products_per_element(ctx, monkeypatch, m, n, density, layout, scaled):
    """mul_ with (alpha, beta) = (1.5, -0.5) and mul_(trans=True) with (-2, 0.25), fast kernels (set_exact(False): 500 x 40 would
    otherwise take the reference-order kernels whatever the layout), plain and column-scaled handle."""
    V, P, c, ref = sparse_case(m, n, density)
    for k, v in LAYOUTS[layout].items():
        monkeypatch.setenv(k, v)
    lsq.set_exact(False)
    try:
        J = lsq.DeviceMatrix(ctx, V if scaled else P)
        if scaled:
            ds = lsq.DeviceVector(ctx, n, c)
            J.set_colscale(ds)
        assert_layout(J.layout(), layout, m, n, P.nnz, scaled)
        judge_both_products(ctx, J, ref, scaled, "%dx%d %s%s" % (m, n, layout, " colscale" if scaled else ""))
        J.free()
    finally:
        lsq.set_exact(None)


@pytest.mark.parametrize("scaled", [False, True])
def test_small_sparse_products_reference_order_per_element(ctx, scaled):
    """500 x 40 as the library runs it by default: the reference-order kernels of lsq_exact.hip."""
    V, P, c, ref = sparse_case(500, 40, 0.5)
    J = lsq.DeviceMatrix(ctx, V if scaled else P)
    if scaled:
        ds = lsq.DeviceVector(ctx, 40, c)
        J.set_colscale(ds)
    judge_both_products(ctx, J, ref, scaled, "500x40 reference order%s" % (" colscale" if scaled else ""))
    J.free()


@functools.lru_cache(maxsize=2)
def dense_case(m, n):
    rng = np.random.default_rng(m * n)
    r, c = ac.product_scales(m, n, m + 2 * n)
    V = np.asfortranarray(rng.standard_normal((m, n)) * r[:, None])
    P = np.asfortranarray(V * c)
    return V, P, c, ProductRef(P, V, r, c, m + n)


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("m,n,exact", [(1025, 129, None), (1025, 129, False), (20000, 12, None)])
def test_dense_products_per_element(ctx, m, n, exact, scaled):
    """1025 x 129 (small enough for the reference-order kernels, which are the default there: both settings run) and
    20000 x 12 (the window-blocked J'y)."""
    V, P, c, ref = dense_case(m, n)
    lsq.set_exact(exact)
    try:
        J = lsq.DeviceMatrix(ctx, V if scaled else P)
        if scaled:
            ds = lsq.DeviceVector(ctx, n, c)
            J.set_colscale(ds)
        judge_both_products(ctx, J, ref, scaled, "dense %dx%d%s%s" % (m, n, "" if exact is None else " fast kernels",
                                                                      " colscale" if scaled else ""))
        J.free()
    finally:
        lsq.set_exact(None)
