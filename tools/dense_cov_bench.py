"""lsq_dense_covariance (lsq_cov_dense.hip) against one Cholesky() lsq_ldiv_damped on the same handle and solver, in the same
run; one JSON line per size.

    python tools/dense_cov_bench.py [--reps 20] [--solver cholesky|qr]

--solver qr: lsq_dense_qr_covariance against one lsq_ldiv of the same QR() solver (for_lm = 0), same sizes, same three calls.
On the certified path the covariance is that solve's launches plus k_cov_xxt + k_cov_stderr and one more wait.

Sizes: 4096 x 512 (C2) and 16384 x 2048 (the C3 size).  Per size three calls are timed, interleaved (solve, cov + stderr,
stderr only, solve, ...) so that a neighbour on the machine hits all three alike: HIP events on the library's stream around the
whole call, 3 warm-up rounds, then the median and minimum of `reps` rounds.  The covariance's last two launches are
stream-ordered, so the closing event -- not the call's return -- ends its window.  Outputs stay on the device (the C entry
point, no download).  Operands: the library's N(0,1)/sqrt(m) generator; the residual is standard normal.
flops: SYRK m n^2, factor / inverse / X X' n^3 / 3 each (the solve: SYRK + factor + 2 n^2 + 2 m n)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lsq_amd as lsq  # noqa: E402

SIZES = [("C2", 4096, 512), ("C3", 16384, 2048)]


class HipEvents:
    """hipEvent pairs on the library's stream, through the HIP runtime the library itself is linked against."""

    def __init__(self, ctx):
        self.hip = C.CDLL("libamdhip64.so")
        lsq.lib().lsq_ctx_stream.restype = C.c_void_p
        self.stream = C.c_void_p(lsq.lib().lsq_ctx_stream(ctx.h))
        self.e0, self.e1 = C.c_void_p(), C.c_void_p()
        for e in (self.e0, self.e1):
            assert self.hip.hipEventCreate(C.byref(e)) == 0

    def timed(self, ctx, fn):
        ctx.sync()
        assert self.hip.hipEventRecord(self.e0, self.stream) == 0
        fn()
        assert self.hip.hipEventRecord(self.e1, self.stream) == 0
        assert self.hip.hipEventSynchronize(self.e1) == 0
        ms = C.c_float(0.0)
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.e0, self.e1) == 0
        return ms.value * 1e-3


def bench(ctx, tag, m, n, reps, warmup=3):
    L = lsq.lib()
    rng = np.random.default_rng(11)
    Jd = lsq.DeviceMatrix(ctx, lsq.synthetic.dense_inputs(m, n, 5).reshape((m, n), order="F"))
    sv = lsq.AllocatedSolver(Jd, lsq.Cholesky(), for_lm=True)
    dx, dy = lsq.DeviceVector(ctx, n), lsq.DeviceVector(ctx, m, rng.standard_normal(m))
    damp_h = 0.05 + rng.random(n)
    dd = lsq.DeviceVector(ctx, n, damp_h)
    dcov, dse = lsq.DeviceVector(ctx, n * n), lsq.DeviceVector(ctx, n)

    def solve():
        dd.set(damp_h)                     # (the solve may clobber damp, as in the reference; the upload is outside the events)
        return lambda: sv.ldiv_(dx, dy, dd)

    calls = {
        "solve": solve,
        "cov_stderr": lambda: (lambda: lsq._lib.check(L.lsq_dense_covariance(sv.h, Jd.h, dy.ptr, dcov.ptr, dse.ptr, None))),
        "stderr_only": lambda: (lambda: lsq._lib.check(L.lsq_dense_covariance(sv.h, Jd.h, dy.ptr, None, dse.ptr, None))),
    }
    evs = HipEvents(ctx)
    t = {k: [] for k in calls}
    paths = {}
    for r in range(warmup + reps):
        for k, prep in calls.items():
            sec = evs.timed(ctx, prep())
            paths[k] = sv.info()["chol_path"]
            if r >= warmup:
                t[k].append(sec)
    out = {"bench": "dense_covariance", "size": tag, "m": m, "n": n, "reps": reps, "chol_path": paths,
           "flops": {"syrk": float(m) * n * n, "factor": n ** 3 / 3.0, "inverse": n ** 3 / 3.0, "xxt": n ** 3 / 3.0}}
    for k in calls:
        out[k] = {"event_median_s": statistics.median(t[k]), "event_min_s": min(t[k])}
    out["cov_over_solve"] = out["cov_stderr"]["event_median_s"] / out["solve"]["event_median_s"]
    out["stderr_over_solve"] = out["stderr_only"]["event_median_s"] / out["solve"]["event_median_s"]
    print(json.dumps(out), flush=True)
    for o in (sv, Jd):
        o.free()


def bench_qr(ctx, tag, m, n, reps, warmup=3):
    L = lsq.lib()
    rng = np.random.default_rng(11)
    Jd = lsq.DeviceMatrix(ctx, lsq.synthetic.dense_inputs(m, n, 5).reshape((m, n), order="F"))
    sv = lsq.AllocatedSolver(Jd, lsq.QR(), for_lm=False)
    dx, dy = lsq.DeviceVector(ctx, n), lsq.DeviceVector(ctx, m, rng.standard_normal(m))
    dcov, dse = lsq.DeviceVector(ctx, n * n), lsq.DeviceVector(ctx, n)
    calls = {
        "solve": lambda: sv.ldiv_(dx, dy),
        "cov_stderr": lambda: lsq._lib.check(L.lsq_dense_qr_covariance(sv.h, Jd.h, dy.ptr, dcov.ptr, dse.ptr, None)),
        "stderr_only": lambda: lsq._lib.check(L.lsq_dense_qr_covariance(sv.h, Jd.h, dy.ptr, None, dse.ptr, None)),
    }
    evs = HipEvents(ctx)
    t = {k: [] for k in calls}
    paths = {}
    for r in range(warmup + reps):
        for k, fn in calls.items():
            sec = evs.timed(ctx, fn)
            info = sv.info()
            paths[k] = "%s/%s" % (info["qr_path"], info["qr_panel"])
            if r >= warmup:
                t[k].append(sec)
    out = {"bench": "dense_qr_covariance", "size": tag, "m": m, "n": n, "reps": reps, "qr_path": paths,
           "flops": {"qr": 2.0 * m * n * n - 2.0 * n ** 3 / 3.0, "inverse": n ** 3 / 3.0, "xxt": n ** 3 / 3.0}}
    for k in calls:
        out[k] = {"event_median_s": statistics.median(t[k]), "event_min_s": min(t[k])}
    out["cov_over_solve"] = out["cov_stderr"]["event_median_s"] / out["solve"]["event_median_s"]
    out["stderr_over_solve"] = out["stderr_only"]["event_median_s"] / out["solve"]["event_median_s"]
    out["cov_minus_solve_s"] = out["cov_stderr"]["event_median_s"] - out["solve"]["event_median_s"]
    print(json.dumps(out), flush=True)
    for o in (sv, Jd):
        o.free()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--solver", choices=["cholesky", "qr"], default="cholesky")
    ap.add_argument("--only", choices=[s[0] for s in SIZES])
    a = ap.parse_args()
    ctx = lsq.default_context()
    for tag, m, n in SIZES:
        if a.only in (None, tag):
            (bench_qr if a.solver == "qr" else bench)(ctx, tag, m, n, a.reps)
