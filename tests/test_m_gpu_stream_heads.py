"""The head of a sliced streaming launch: the gather vector staged by LDS-DMA, the first slice requested ahead of the barrier.

k_sell_rows (an unscaled gather vector) and k_sell_cols stage their vector global -> LDS with no register in between
(lsq_sell.h: sell_stage_dma) and request every wave's first slice before the wait that retires the staged vector.  What can go
wrong there shows at SMALL shapes, chosen below:

  * n = 1, 2, 63, 127, 129, 2049: fewer 16-byte chunks than one wave, a partly filled wave, an odd n (the single double behind
    the chunks), more than one chunk per thread;
  * m = 589 with LSQ_SELL_ROWS=128 and LSQ_SELL_GROWS=256: five row blocks, three gather windows of J'y, the last one with 77
    rows (odd, fewer than 1024: zero fill behind a DMA with a single-double tail);
  * the last row and the last column hold an entry (a tail element that was never staged shows there);
  * rows 5 is full (n >= 18: its slice is the first of its block and has more than 8 pairs), rows 256..511 are empty (an
    empty first slice in J x, a whole gather window of J'y without entries), the other rows have 0..7 entries at random, so
    first slices with an odd and with an even number of entries both occur.

Per shape, plain and column-scaled handle (the scaled J x keeps the register staging; the scaled J'y is DMA-staged).  That both
sliced layouts of a handle were built is known from an LSMR solve on it: the three-launch driver (info()["lsmr_path"]) runs only
on a handle whose sliced rows and sliced columns are both active.
  1. every output of mul_ and mul_(trans=True) within the any-order bound of tests/test_i_gpu_accuracy_products.py (its judge, its
     reference class, imported);
  2. two consecutive calls with DIFFERENT vectors on one handle give, bit for bit, what the same calls give on fresh handles: a
     gather that ran before the DMA had landed would read the previous call's vector or stale LDS.
A vector at an 8-byte-but-not-16-byte offset (DeviceVector.borrow one element into an allocation) takes the register staging:
one product each way against the aligned result, bit for bit.

The solve: LM+LSMR of the tanh model at 4000 x 129 with the sliced layouts forced (the column-scaled handle; start residual
pass, J'u passes and the gradient pass on the new heads), bit-equal to itself with every launch waited for and under 100 us
launch jitter, and equal in counts and to 1e-12 in ssr / iterates to the two-pass tail (LSQ_NO_PAIR_TAIL=1), the comparator and
tolerances of tests/test_l_gpu_solve_ends.py and test_lm_pair_tail_matches_the_two_passes.  TanhProblem.paths()
(lsq_model_paths) tells what ran: both sliced layouts built, the three-launch LSMR driver, one launch of the pair tail per LM
step (none under LSQ_NO_PAIR_TAIL=1).

Those comparisons are the library against itself on the same heads.  The independent reference is the CPU oracle on the same
pattern, values and right-hand side, as tests/test_a_gpu_contract.py::test_tanh_model_matches_oracle builds it: iterations,
mul_calls, f_calls, g_calls, converged and the inner counts per step equal; ssr to 1e-12 relative (the tolerance of
tests/test_l_gpu_solve_ends.py: at a minimum of ssr a difference dx of the iterates enters as g'dx + O(dx^2), far below the
rounding of a sum of 4000 squares, which is at most 4000 * 2^-53 = 4.4e-13 relative and typically 1e-15); every traced iterate
to 1e-8 * max(1, |x|), test_tanh_model_matches_oracle's bound."""
import ctypes
import functools

import numpy as np
import pytest

import accuracy_common as ac
from gpu_common import OPT, SOL, lsq
from oracle import oracle as O
from test_i_gpu_accuracy_products import ProductRef, judge_both_products

pytestmark = pytest.mark.gpu

M = 589
NS = (1, 2, 63, 127, 129, 2049)
ENV = {"LSQ_SELL_FORCE": "1", "LSQ_SELL_ROWS": "128", "LSQ_SELL_GROWS": "256"}
L = lsq._lib


@functools.lru_cache(maxsize=None)
def case(n):
    import scipy.sparse as sp
    rng = np.random.default_rng(1000 + n)
    S = sp.random(M, n, density=min(1.0, 3.5 / n), format="lil", random_state=rng, data_rvs=rng.standard_normal)
    S[5, :] = rng.standard_normal(n)              # a full row: first slice of its block
    S[256:512, :] = 0                             # a gather window of J'y and two row blocks of J x without entries
    S[M - 1, n - 1] = 1.25                        # the last row and the last column are used
    S[0, 0] = -0.75
    S = S.tocsc()
    S.sort_indices()
    S.eliminate_zeros()
    r, c = ac.product_scales(M, max(n, 2), M + 2 * n)      # (a grading of ONE value is undefined: n = 1 takes the first of two)
    c = c[:n]
    V = (S.multiply(r[:, None])).tocsc()
    P = (V.multiply(c[None, :])).tocsc()
    for A in (V, P):
        A.sort_indices()
    assert np.array_equal(V.indices, P.indices) and np.all(P.data != 0) and np.all(np.isfinite(P.data))
    return V, P, c, ProductRef(P.toarray(), V.toarray(), r, c, M * n + 1)


def handle(ctx, n, scaled):
    V, P, c, _ = case(n)
    J = lsq.DeviceMatrix(ctx, V if scaled else P)
    keep = None
    if scaled:
        keep = lsq.DeviceVector(ctx, n, c)
        J.set_colscale(keep)
    return J, keep


def both(ctx, J, n, seed):
    """J x and J'y for vectors drawn from `seed`: (m values, n values)."""
    rng = np.random.default_rng(seed)
    x, y = rng.standard_normal(n), rng.standard_normal(M)
    a = lsq.mul_(lsq.DeviceVector(ctx, M, np.zeros(M)), J, lsq.DeviceVector(ctx, n, x), 1.0, 0.0).get()
    b = lsq.mul_(lsq.DeviceVector(ctx, n, np.zeros(n)), J, lsq.DeviceVector(ctx, M, y), 1.0, 0.0, trans=True).get()
    return a, b


def both_layouts_built(ctx, J, n):
    """DeviceMatrix.layout() shows what ENV asked for -- sliced rows in blocks of 128 with one column window, sliced columns
    with three gather windows of 256 rows -- and an LSMR solve on J took the three-launch driver, which needs both."""
    lay = J.layout()
    if not (lay["srows"]["active"] and lay["scols"]["active"] and
            (lay["srows"]["ncw"], lay["srows"]["wrows"], lay["scols"]["ngw"]) == (1, 128, 3)):
        return False
    sv = lsq.AllocatedSolver(J, lsq.LSMR(), for_lm=False)
    try:
        y = np.random.default_rng(3).standard_normal(M)
        sv.ldiv_(lsq.DeviceVector(ctx, n, np.zeros(n)), lsq.DeviceVector(ctx, M, y))
        return sv.info()["lsmr_path"] == "three-launch"
    finally:
        sv.free()


@pytest.fixture()
def sliced(monkeypatch):
    for k, v in ENV.items():
        monkeypatch.setenv(k, v)
    lsq.set_exact(False)
    yield
    lsq.set_exact(None)


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("n", NS)
def test_products_per_element(ctx, sliced, n, scaled):
    J, keep = handle(ctx, n, scaled)
    assert both_layouts_built(ctx, J, n)
    judge_both_products(ctx, J, case(n)[3], scaled, "589x%d stream heads%s" % (n, " colscale" if scaled else ""))
    J.free()


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("n", NS)
def test_consecutive_calls_equal_fresh_handles(ctx, sliced, n, scaled):
    J, keep = handle(ctx, n, scaled)
    first, second = both(ctx, J, n, 7), both(ctx, J, n, 8)
    assert both_layouts_built(ctx, J, n)
    J.free()
    for seed, got in ((8, second), (7, first)):
        F, fkeep = handle(ctx, n, scaled)
        want = both(ctx, F, n, seed)
        F.free()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (n, scaled, seed)
    assert n == 1 or not np.array_equal(first[0], second[0])


@pytest.mark.parametrize("n", [129, 2049])
def test_unaligned_vectors_take_the_register_staging(ctx, sliced, n):
    J, _ = handle(ctx, n, False)
    assert both_layouts_built(ctx, J, n)
    rng = np.random.default_rng(n)
    x, y = rng.standard_normal(n), rng.standard_normal(M)
    want_a = lsq.mul_(lsq.DeviceVector(ctx, M, np.zeros(M)), J, lsq.DeviceVector(ctx, n, x), 1.0, 0.0).get()
    want_b = lsq.mul_(lsq.DeviceVector(ctx, n, np.zeros(n)), J, lsq.DeviceVector(ctx, M, y), 1.0, 0.0, trans=True).get()
    bx, by = lsq.DeviceVector(ctx, n + 1, np.concatenate(([9.0], x))), lsq.DeviceVector(ctx, M + 1, np.concatenate(([9.0], y)))
    px, py = ctypes.cast(bx.ptr, ctypes.c_void_p).value, ctypes.cast(by.ptr, ctypes.c_void_p).value
    assert px % 16 == 0 and py % 16 == 0
    ux, uy = lsq.DeviceVector.borrow(ctx, n, ctypes.c_void_p(px + 8)), lsq.DeviceVector.borrow(ctx, M, ctypes.c_void_p(py + 8))
    got_a = lsq.mul_(lsq.DeviceVector(ctx, M, np.zeros(M)), J, ux, 1.0, 0.0).get()
    got_b = lsq.mul_(lsq.DeviceVector(ctx, n, np.zeros(n)), J, uy, 1.0, 0.0, trans=True).get()
    J.free()
    assert np.array_equal(got_a, want_a) and np.array_equal(got_b, want_b)


SM, SN, SPER, SSEED = 4000, 129, 300, 31


def _solve(ctx, monkeypatch, env=None, oracle=False):
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    try:
        pr = lsq.synthetic.TanhProblem(SM, SN, sparse=True, per_col=SPER, seed=SSEED, ctx=ctx)
        try:
            pr.reset()
            r = pr.optimize(L.LEVENBERG_MARQUARDT, L.LSMR, trace=True)
            out = [r.iterations, r.converged, r.f_calls, r.g_calls, r.mul_calls, r.lsmr_iterations,
                   np.array(r.trace["inner"]), np.array(r.trace["accept"]), r.ssr, np.array(r.trace["ssr"]), r.minimizer,
                   pr.fcur.get()]
            paths = pr.paths()
            assert paths["sliced_rows"] and paths["sliced_cols"] and paths["lsmr_path"] == "three-launch", paths
            # (one tail per LM step: the trial residual of every step goes through it)
            assert paths["pair_tails"] == (0 if env and "LSQ_NO_PAIR_TAIL" in env else r.iterations), (paths, r.iterations)
            if oracle:
                A = O.Mat(csc=(SM, SN, pr.colptr, pr.rowval, pr.A))
                Jo = O.Mat(csc=(SM, SN, pr.colptr, pr.rowval, np.zeros_like(pr.A)))
                f, g, ud, keep = O.tanh_model(A, pr.b)
                ro = O.optimize(OPT["lm"][1], SOL["lsmr"][1], Jo, np.zeros(SN), f, g, ud=ud)
                print("oracle: iterations %d/%d mul_calls %d/%d ssr %.17g/%.17g rel %.3e" % (
                    r.iterations, ro.iterations, r.mul_calls, ro.mul_calls, r.ssr, ro.ssr, abs(r.ssr - ro.ssr) / ro.ssr))
                print("oracle: max |x_k - x_k oracle| / max(1, |x_k|) over the steps: %.3e" % max(
                    np.max(np.abs(r.trace["x"][k] - ro.trace["x"][k])) / max(1.0, np.max(np.abs(ro.trace["x"][k])))
                    for k in range(min(r.iterations, ro.iterations))))
                assert (r.iterations, r.mul_calls, r.f_calls, r.g_calls, r.converged) == \
                       (ro.iterations, ro.mul_calls, ro.f_calls, ro.g_calls, ro.converged)
                assert np.array_equal(r.trace["inner"], ro.trace["inner"])
                assert r.ssr == pytest.approx(ro.ssr, rel=1e-12)
                for k in range(ro.iterations):
                    xr = ro.trace["x"][k]
                    assert np.max(np.abs(r.trace["x"][k] - xr)) <= 1e-8 * max(1.0, np.max(np.abs(xr))), k
            return out
        finally:
            pr.close()
    finally:
        for k in (env or {}):
            monkeypatch.delenv(k)


def test_lm_lsmr_solve_on_forced_sliced_layouts(ctx, monkeypatch):
    for k, v in {"LSQ_SELL_FORCE": "1", "LSQ_SELL_ROWS": "512", "LSQ_SELL_GROWS": "1000"}.items():
        monkeypatch.setenv(k, v)
    prev = lsq.debug_get()
    lsq.set_exact(False)        # (a problem this small would otherwise take the reference-order kernels)
    try:
        lsq.debug_set(0, 0)
        normal = _solve(ctx, monkeypatch, oracle=True)
        assert normal[1] and normal[0] >= 2, normal[:6]
        for jitter, serial in ((0, 1), (100, 0)):
            lsq.debug_set(jitter, serial)
            other = _solve(ctx, monkeypatch)
            for k, (u, v) in enumerate(zip(normal, other)):
                assert np.array_equal(u, v) if isinstance(u, np.ndarray) else u == v, (jitter, serial, k)
        lsq.debug_set(0, 0)
        two = _solve(ctx, monkeypatch, {"LSQ_NO_PAIR_TAIL": "1"})
    finally:
        lsq.debug_set(prev[0], prev[1])
        lsq.set_exact(None)
    assert normal[:6] == two[:6]
    assert np.array_equal(normal[6], two[6]) and np.array_equal(normal[7], two[7])
    assert normal[8] == pytest.approx(two[8], rel=1e-12) and np.allclose(normal[9], two[9], rtol=1e-12, atol=0)
    assert np.max(np.abs(normal[10] - two[10])) <= 1e-12
    assert np.max(np.abs(normal[11] - two[11])) <= 1e-12 * max(1.0, np.max(np.abs(two[11])))
