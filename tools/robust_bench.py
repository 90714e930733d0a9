"""Robust losses and observation weights (csrc/lsq_loss.hip, lsq_mat_scale_rows in csrc/lsq_sparse.hip), measured on the
benchmark's sparse pattern (10^6 x 10^4 with 1000 entries per column unless told otherwise) and on a C3-sized dense handle
(16384 x 2048).  One JSON line:

    copy_GBps                      a device-to-device copy of 512 MiB, read + write counted: the rate the bounds are taken at
    sparse / dense . scale_rows_ms lsq_mat_scale_rows (the scaling launch and the rebuild of every mirror that follows it)
                   . refresh_ms    lsq_mat_refresh alone on the same handle: that rebuild
                   . scale_only_ms the difference: the scaling pass itself
                   . bound_ms      8 B read + 8 B write per stored value (+ 4 B of rowval on plain CSC) at copy_GBps
                   . over_bound    scale_only_ms / bound_ms
    loss_eval . <kind> . ms        lsq_loss_eval on --eval-rows rows, both outputs, no sigmas: 24 B per row
                       . over_bound against that traffic at copy_GBps
    fit                            LevenbergMarquardt(LSMR()) with loss="huber" through lsq_loss_f / lsq_loss_g on a host-callback
                                   problem (r = A tanh(x) - b with displaced rows, --fit-m x --fit-n), a fixed number of outer
                                   iterations, against the same loop driven by the host twin (lsq_amd.robust_twin): seconds of
                                   both, and whether x came out with the same bits

Wall-clock times around stream synchronisations; medians of --reps after one warm-up.  Needs a device: no figure is produced
without one."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lsq_amd as lsq  # noqa: E402


def median_ms(ctx, call, reps):
    call()
    ctx.sync()
    ts = []
    for _ in range(reps):
        ctx.sync()
        t0 = time.perf_counter()
        call()
        ctx.sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def copy_rate(ctx):
    L, check = lsq.lib(), lsq._lib.check
    nb = 512 << 20
    src, dst = C.c_void_p(), C.c_void_p()
    check(L.lsq_malloc(ctx.h, nb, C.byref(src)))
    check(L.lsq_malloc(ctx.h, nb, C.byref(dst)))
    ms = median_ms(ctx, lambda: check(L.lsq_d2d(ctx.h, dst, src, nb)), 10)
    L.lsq_free(ctx.h, src)
    L.lsq_free(ctx.h, dst)
    return 2 * nb / (ms * 1e-3) / 1e9


def handle_figures(ctx, J, bytes_per_value, rate, reps):
    L, check = lsq.lib(), lsq._lib.check
    w = lsq.DeviceVector(ctx, J.m, np.ones(J.m))            # (factors of 1: the values survive any number of repetitions)
    scale = median_ms(ctx, lambda: check(L.lsq_mat_scale_rows(J.h, w.ptr)), reps)
    refresh = median_ms(ctx, lambda: check(L.lsq_mat_refresh(J.h)), reps)
    bound = bytes_per_value * J.nnz / (rate * 1e9) * 1e3
    return {"shape": [J.m, J.n], "stored_values": int(J.nnz), "layout": {k: v for k, v in J.layout().items() if k in ("kind", "srows", "scols", "nwin")},
            "scale_rows_ms": scale, "refresh_ms": refresh, "scale_only_ms": scale - refresh, "bound_ms": bound,
            "over_bound": (scale - refresh) / bound}


def fit_figures(ctx, m, n, per_col, iterations):
    colptr, rowval, nzval = lsq.synthetic.sparse_inputs(m, n, per_col, lsq.synthetic.BASE_SEED)
    A = sp.csc_matrix((nzval, rowval, colptr), shape=(m, n))
    R = A.tocsr()
    cols = np.repeat(np.arange(n), np.diff(colptr))
    rng = np.random.default_rng(5)
    b = R @ np.tanh(rng.uniform(-1.0, 1.0, n)) + 0.01 * rng.standard_normal(m)
    out_rows = rng.choice(m, size=m // 20, replace=False)
    b[out_rows] += 5.0
    sigma = 10.0 ** rng.uniform(-1.0, 0.0, m)

    def f_(o, x):
        o[:] = R @ np.tanh(x) - b

    def g_(J, x):
        J.data[:] = nzval * (1.0 - np.tanh(x) ** 2)[cols]

    def problem(f, g):
        return lsq.LeastSquaresProblem(x=np.zeros(n), y=np.zeros(m), f_=f, g_=g, J=sp.csc_matrix((np.zeros(len(nzval)), rowval, colptr), shape=(m, n)))

    kw = dict(x_tol=0.0, f_tol=0.0, g_tol=0.0, iterations=iterations)
    opt = lsq.LevenbergMarquardt(lsq.LSMR())
    res = {}
    for rep in range(2):            # (the first pair warms up the code objects)
        pa = problem(f_, g_)
        t0 = time.perf_counter()
        ra = lsq.optimize_(pa, opt, loss="huber", f_scale=1.0, sigma=sigma, **kw)
        ta = time.perf_counter() - t0
        pb = problem(*lsq.robust_twin(f_, g_, "huber", 1.0, sigma))
        t0 = time.perf_counter()
        rb = lsq.optimize_(pb, opt, **kw)
        tb = time.perf_counter() - t0
        res = {"shape": [m, n], "stored_values": int(len(nzval)), "outer_iterations": ra.iterations, "g_calls": ra.g_calls,
               "device_wrapper_seconds": ta, "host_twin_seconds": tb, "loop_seconds_device_wrapper": ra.seconds,
               "loop_seconds_host_twin": rb.seconds, "same_bits": bool(np.array_equal(pa.x, pb.x)), "outliers": ra.outliers,
               "ssr": ra.ssr}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=1_000_000)
    ap.add_argument("--n", type=int, default=10_000)
    ap.add_argument("--per-col", type=int, default=1000)
    ap.add_argument("--dense-m", type=int, default=16384)
    ap.add_argument("--dense-n", type=int, default=2048)
    ap.add_argument("--eval-rows", type=int, default=16_000_000)
    ap.add_argument("--fit-m", type=int, default=200_000)
    ap.add_argument("--fit-n", type=int, default=2_000)
    ap.add_argument("--fit-per-col", type=int, default=1000)
    ap.add_argument("--fit-iterations", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    ctx = lsq.default_context()
    rate = copy_rate(ctx)
    out = {"copy_GBps": rate}

    colptr, rowval, nzval = lsq.synthetic.sparse_inputs(a.m, a.n, a.per_col, lsq.synthetic.BASE_SEED)
    J = lsq.DeviceMatrix(ctx, sp.csc_matrix((nzval, rowval, colptr), shape=(a.m, a.n)))
    out["sparse"] = handle_figures(ctx, J, 20, rate, a.reps)
    J.free()
    D = lsq.DeviceMatrix(ctx, lsq.synthetic.dense_inputs(a.dense_m, a.dense_n, 1).reshape((a.dense_m, a.dense_n), order="F"))
    out["dense"] = handle_figures(ctx, D, 16, rate, a.reps)
    D.free()

    rows = a.eval_rows
    f = lsq.DeviceVector(ctx, rows, 3.0 * np.random.default_rng(2).standard_normal(rows))
    rt, rowf = lsq.DeviceVector(ctx, rows), lsq.DeviceVector(ctx, rows)
    out["loss_eval"] = {"rows": rows}
    for kind in lsq.LOSSES:
        lo = lsq.Loss(ctx, kind, 1.0, rows)
        ms = median_ms(ctx, lambda: lo.eval(f, rt, rowf), a.reps)
        bound = 24 * rows / (rate * 1e9) * 1e3
        out["loss_eval"][kind] = {"ms": ms, "bound_ms": bound, "over_bound": ms / bound}
        lo.free()
    for v in (f, rt, rowf):
        v.free()

    out["fit"] = fit_figures(ctx, a.fit_m, a.fit_n, a.fit_per_col, a.fit_iterations)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
