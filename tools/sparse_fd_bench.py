"""Coloured central differences on a general sparse pattern (csrc/lsq_fd.hip: lsq_mat_set_fd_colouring + lsq_fd_jacobian),
measured on the C4 pattern (synthetic.TanhProblem, 10^6 x 10^4 with 1000 entries per column unless told otherwise) with the
device f! of the built-in model (lsq_model_f).  One JSON line:

    colours, max_row_count     what the greedy colouring found against its lower bound
    colouring_seconds          host seconds of lsq_csc_greedy_colouring (the C entry, pattern in host arrays)
    attach_seconds             lsq_mat_set_fd_colouring(NULL): pattern download, colouring, tables, upload
    jacobian_ms                one lsq_fd_jacobian with the device f! (2 colours evaluations, colours + 1 launches, refresh)
    launches_ms                the same call with an f! that does nothing: the library's launches (and the refresh) alone
    launches_only_ms           launches_ms minus the refresh of the mirrors (lsq_mat_refresh timed on its own)
    bound_ms                   28 B per stored entry + 16 B per column and colour touched, at the measured copy rate
    copy_GBps                  that rate: a device-to-device copy of 512 MiB, read + write counted
    g_pass_ms                  one all-entries device g! (lsq_model_g on a handle that is multiplied out) over the same pattern
    launches_over_g_pass       launches_only_ms / g_pass_ms
    max_rel_diff               max |fd - analytic| / max |analytic| over the stored entries, analytic = lsq_model_g's values
    max_rel_diff_entrywise     max over the entries of |fd - analytic| / |analytic|

Wall-clock times around stream synchronisations; medians of --reps after one warm-up."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=1_000_000)
    ap.add_argument("--n", type=int, default=10_000)
    ap.add_argument("--per-col", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    L = lsq.lib()
    check = lsq._lib.check
    ctx = lsq.default_context()
    m, n = a.m, a.n
    inputs = lsq.synthetic.sparse_inputs(m, n, a.per_col, lsq.synthetic.BASE_SEED)
    colptr, rowval, nzval = inputs
    nnz = len(nzval)
    # the model keeps A aside and J holds plain values (a column-scaled handle is refused by lsq_fd_jacobian)
    saved = os.environ.get("LSQ_NO_COLSCALE")
    os.environ["LSQ_NO_COLSCALE"] = "1"
    try:
        pr = lsq.synthetic.TanhProblem(m, n, sparse=True, per_col=a.per_col, seed=0, ctx=ctx, inputs=inputs)
    finally:
        if saved is None:
            os.environ.pop("LSQ_NO_COLSCALE", None)
        else:
            os.environ["LSQ_NO_COLSCALE"] = saved
    out = {"workload": "sparse CSC %dx%d, nnz=%d, tanh model, device f!" % (m, n, nnz), "paths": pr.paths()}

    ip = lambda v: v.ctypes.data_as(lsq._lib.c_ip)
    colour, nc = np.zeros(n, dtype=np.int32), C.c_int(0)
    t0 = time.perf_counter()
    check(L.lsq_csc_greedy_colouring(m, n, ip(colptr), ip(rowval), ip(colour), C.byref(nc)))
    out["colouring_seconds"] = time.perf_counter() - t0
    out["colours"] = nc.value
    out["max_row_count"] = int(np.bincount(rowval, minlength=m).max())
    t0 = time.perf_counter()
    check(L.lsq_mat_set_fd_colouring(pr.J, None, C.byref(nc)))
    out["attach_seconds"] = time.perf_counter() - t0
    assert nc.value == out["colours"]

    x = lsq.DeviceVector(ctx, n, np.random.default_rng(1).uniform(-0.5, 0.5, n))
    F, G = L.lsq_model_f(), L.lsq_model_g()
    # an f! that does nothing and costs nothing: libc's sched_yield() returns 0 and ignores the three arguments (a Python
    # callback would cost more per call than the launch it stands between)
    nothing = lsq._lib.F_CALLBACK(C.cast(C.CDLL(None).sched_yield, C.c_void_p).value)
    vals = lambda: (check(L.lsq_mat_get_values(pr.J, buf.ctypes.data_as(lsq._lib.c_dp))), buf.copy())[1]
    buf = np.zeros(nnz)

    # the analytic values, and the time of one all-entries g! pass
    assert G(pr.J, x.ptr, pr.model) == 0
    analytic = vals()
    out["g_pass_ms"] = median_ms(ctx, lambda: G(pr.J, x.ptr, pr.model), max(a.reps, 10))

    check(L.lsq_fd_jacobian(ctx.h, pr.J, x.ptr, F, pr.model))
    fd = vals()
    diff = np.abs(fd - analytic)
    out["max_rel_diff"] = float(diff.max() / np.abs(analytic).max())
    nz = analytic != 0
    out["max_rel_diff_entrywise"] = float((diff[nz] / np.abs(analytic[nz])).max())

    out["jacobian_ms"] = median_ms(ctx, lambda: check(L.lsq_fd_jacobian(ctx.h, pr.J, x.ptr, F, pr.model)), a.reps)
    out["launches_ms"] = median_ms(ctx, lambda: check(L.lsq_fd_jacobian(ctx.h, pr.J, x.ptr, nothing, None)), a.reps)
    refresh_ms = median_ms(ctx, lambda: check(L.lsq_mat_refresh(pr.J)), max(a.reps, 10))
    out["refresh_ms"] = refresh_ms
    out["launches_only_ms"] = out["launches_ms"] - refresh_ms

    nb = 512 << 20
    src, dst = C.c_void_p(), C.c_void_p()
    check(L.lsq_malloc(ctx.h, nb, C.byref(src)))
    check(L.lsq_malloc(ctx.h, nb, C.byref(dst)))
    copy_ms = median_ms(ctx, lambda: check(L.lsq_d2d(ctx.h, dst, src, nb)), 10)
    L.lsq_free(ctx.h, src)
    L.lsq_free(ctx.h, dst)
    out["copy_GBps"] = 2 * nb / (copy_ms * 1e-3) / 1e9
    bound_bytes = 28 * nnz + 16 * 2 * n + 8 * 3 * n          # entries; x+ / x- restored and set once per column; begin
    out["bound_bytes"] = bound_bytes
    out["bound_ms"] = bound_bytes / (out["copy_GBps"] * 1e9) * 1e3
    out["launches_over_bound"] = out["launches_only_ms"] / out["bound_ms"]
    out["launches_over_g_pass"] = out["launches_only_ms"] / out["g_pass_ms"]
    out["launch_us_per_colour"] = out["launches_only_ms"] * 1e3 / max(out["colours"], 1)
    print(json.dumps(out))
    pr.close()


if __name__ == "__main__":
    main()
