"""lsq_sparse_gram / lsq_sparse_covariance (lsq_cov_sparse.hip) on the C4 pattern of synthetic.py (m = 10^6, n = 10^4,
1000 entries per column: the headline benchmark's problem), one JSON line.

    python tools/sparse_cov_bench.py [--m 1000000 --n 10000 --per-col 1000] [--reps 3] [--pairs N] [--only-cov]

What is timed, all in one process on one handle -- the benchmark's own TanhProblem after one LM+LSMR fit, so J is the Jacobian
at the solution, a column-scaled handle as the fit leaves it:
    fit            one LevenbergMarquardt(LSMR()) fit from x0 = 0 with the default tolerances (the host clock around the call,
                   which ends in a synchronise), after a warm-up fit
    gram           k_sp_gram alone (lsq_sparse_gram), device events, `reps` rounds after a warm-up: median and minimum
    pairs          the only route to J'J the library had before: n pairs of products J'(J e_j) through lsq_mul, column j written
                   straight into column j of an n x n buffer; e_j is a window of one 2n-vector with a single 1, so the loop
                   holds nothing but the 2n lsq_mul calls.  Device events around `--pairs` pairs (default: all n) after 64
                   warm-up pairs, scaled to n pairs when fewer were run (stated in the output).
    cov / stderr   lsq_sparse_covariance with and without d_cov, device events, `reps` rounds interleaved with gram
The two Gram matrices are compared on 16 sampled columns (relative to the column's largest entry).
Traffic bound of the kernel: the gathered row bytes -- per stored entry of column j the entries of its row up to column j, 16 B
each (index, map, value: 4 + 4 + 8), counted exactly from the pattern on the host -- plus the 8 (n^2 + n) / 2 bytes stored, over
the HBM rate given with --hbm-gbs (default 8000, the MI355X datasheet figure).
--only-cov: nothing but two covariance calls (for a kernel trace of the stages: factorisation, inverse, k_cov_xxt,
k_cov_stderr; run it under the profiler's kernel trace, in a run of its own)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lsq_amd as lsq  # noqa: E402
from dense_cov_bench import HipEvents  # noqa: E402


class Handle:
    """The benchmark problem's raw Jacobian handle with what AllocatedSolver asks of a DeviceMatrix."""

    def __init__(self, pr):
        self.ctx, self.h, self.m, self.n, self.sparse = pr.ctx, pr.J, pr.m, pr.n, True
        self.blockdiag = self.bordered = None


def gathered_bytes(m, n, colptr, rowval):
    """Sum over the stored entries (i, j) of the number of entries of row i with column <= j, times 16 B."""
    cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(colptr))
    order = np.lexsort((cols, rowval))                    # by row, then column
    rows_sorted = rowval[order]
    start = np.searchsorted(rows_sorted, np.arange(m))    # first position of every row
    rank = np.arange(len(order)) - start[rows_sorted]     # position inside its row = entries with a smaller column
    return 16 * int(np.sum(rank + 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=1000000)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--per-col", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=0)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--only-cov", action="store_true")
    a = ap.parse_args()
    m, n = a.m, a.n
    ctx = lsq.default_context()
    L = lsq.lib()
    chk = lsq._lib.check
    LM, LSMR = lsq._lib.LEVENBERG_MARQUARDT, lsq._lib.LSMR
    pr = lsq.synthetic.TanhProblem(m, n, sparse=True, per_col=a.per_col, ctx=ctx)
    fit = []
    for _ in range(2):                                     # (the second one is the timed one)
        pr.reset()
        t0 = time.perf_counter()
        r = pr.optimize(LM, LSMR, iterations=50, fetch_x=False)
        ctx.sync()
        fit.append(time.perf_counter() - t0)
    Jd = Handle(pr)
    sv = lsq.AllocatedSolver(Jd, lsq.LSMR(), for_lm=True)
    dse = lsq.DeviceVector(ctx, n)
    dcov = lsq.DeviceVector(ctx, n * n)
    evs = HipEvents(ctx)
    cov_call = lambda: chk(L.lsq_sparse_covariance(sv.h, Jd.h, pr.fcur.ptr, dcov.ptr, dse.ptr, None))
    se_call = lambda: chk(L.lsq_sparse_covariance(sv.h, Jd.h, pr.fcur.ptr, None, dse.ptr, None))
    if a.only_cov:
        for _ in range(2):
            cov_call()
        ctx.sync()
        print(json.dumps({"bench": "sparse_covariance", "only_cov": True, "m": m, "n": n, "chol_path": sv.info()["chol_path"]}))
        return
    dG = lsq.DeviceVector(ctx, n * n)
    gram_call = lambda: chk(L.lsq_sparse_gram(Jd.h, None, dG.ptr))
    calls = {"gram": gram_call, "cov_stderr": cov_call, "stderr_only": se_call}
    t = {k: [] for k in calls}
    for rnd in range(1 + a.reps):
        for k, fn in calls.items():
            sec = evs.timed(ctx, fn)
            if rnd >= 1:
                t[k].append(sec)
    # the route through the products
    npairs = a.pairs if 0 < a.pairs < n else n
    z = np.zeros(2 * n)
    z[n] = 1.0
    dz, dt, dP = lsq.DeviceVector(ctx, 2 * n, z), lsq.DeviceVector(ctx, m), lsq.DeviceVector(ctx, n * n)
    zb, pb = dz.ptr.value, dP.ptr.value

    def pairs(j0, j1):
        for j in range(j0, j1):
            chk(L.lsq_mul(Jd.h, 0, 1.0, C.c_void_p(zb + 8 * (n - j)), 0.0, dt.ptr))
            chk(L.lsq_mul(Jd.h, 1, 1.0, dt.ptr, 0.0, C.c_void_p(pb + 8 * j * n)))

    evs.timed(ctx, lambda: pairs(0, min(64, n)))
    t_pairs = evs.timed(ctx, lambda: pairs(n - npairs, n))          # (the last columns: the ones the comparison samples)
    # both routes on sampled columns
    worst = 0.0
    for j in sorted(set(int(c) for c in np.linspace(n - npairs, n - 1, 16))):
        ca, cb = np.empty(n), np.empty(n)
        chk(L.lsq_d2h(ctx.h, ca.ctypes.data_as(C.c_void_p), C.c_void_p(dG.ptr.value + 8 * j * n), 8 * n))
        chk(L.lsq_d2h(ctx.h, cb.ctypes.data_as(C.c_void_p), C.c_void_p(pb + 8 * j * n), 8 * n))
        worst = max(worst, float(np.max(np.abs(ca[:j + 1] - cb[:j + 1])) / np.max(np.abs(cb[:j + 1]))))
    gb = gathered_bytes(m, n, pr.colptr.astype(np.int64), pr.rowval.astype(np.int64))
    sb = 8 * (n * n + n) // 2
    bound_s = (gb + sb) / (a.hbm_gbs * 1e9)
    out = {"bench": "sparse_covariance", "m": m, "n": n, "nnz": int(pr.nnz), "reps": a.reps, "chol_path": sv.info()["chol_path"],
           "fit": {"wall_s": fit[1], "warmup_wall_s": fit[0], "outer_iterations": r.iterations, "lsmr_iterations": r.lsmr_iterations},
           "pairs": {"run": npairs, "event_s": t_pairs, "scaled_to_n_s": t_pairs * n / npairs},
           "traffic": {"gathered_bytes": gb, "stored_bytes": sb, "hbm_gbs_assumed": a.hbm_gbs, "bound_s": bound_s},
           "gram_vs_pairs_max_rel_diff": worst}
    for k in calls:
        out[k] = {"event_median_s": statistics.median(t[k]), "event_min_s": min(t[k])}
    g = out["gram"]["event_median_s"]
    out["pairs_over_gram"] = out["pairs"]["scaled_to_n_s"] / g
    out["gram_over_traffic_bound"] = g / bound_s
    out["gram_achieved_gbs"] = (gb + sb) / g / 1e9
    out["after_gram_s"] = {"factor_inverse_stderr": out["stderr_only"]["event_median_s"] - g,
                           "xxt": out["cov_stderr"]["event_median_s"] - out["stderr_only"]["event_median_s"]}
    out["cov_over_fit"] = out["cov_stderr"]["event_median_s"] / fit[1]
    out["stderr_over_fit"] = out["stderr_only"]["event_median_s"] / fit[1]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
