"""lsq_dense_qr_leverage (lsq_leverage.hip) against one lsq_ldiv of the same QR() solver on the same operand, and its hot kernel
k_lev_tall against k_bqc_tall (lsq_cov_bordered.hip) on a product of the same flop count; one JSON line per size.

    python tools/leverage_bench.py [--reps 20] [--only C2|C3]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/leverage_bench.py --kernels 10 [--only C2|C3]

Sizes: 4096 x 512 (C2) and 16384 x 2048 (the C3 size), J's own rows.  Default mode: three calls are timed, interleaved (solve,
leverages alone, leverages + se + studentized + Cook, solve, ...) so that a neighbour on the machine hits all alike: HIP events
on the library's stream around the whole call, 3 warm-up rounds, then the median and minimum of `reps` rounds.  The launches
behind the rank are stream-ordered, so the closing event -- not the call's return -- ends the window.  Outputs stay on the
device (the C entry point, no download).  Operands: the library's N(0,1)/sqrt(m) generator; the residual is standard normal.
flops: the factorisation 2 m n^2 - 2/3 n^3, the product m n^2 (only K <= Jt of the triangular X contributes).

--kernels N: nothing is timed here.  N leverage calls and N lsq_bordered_qr_covariance calls (d_cross alone) on a bordered handle
whose tall product P = T Cgg has the same flop count -- 2 (B nb) ng^2 = m n^2 with ng = n, nb = 64, B = m / 128 -- in ONE
process, for the profiler's kernel trace: both kernels are tall fp64 MFMA products with the same tile, and their per-launch
times come from the same run.  The JSON line carries the flop counts to divide by."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lsq_amd as lsq  # noqa: E402
from dense_cov_bench import SIZES, HipEvents  # noqa: E402


def dense_setup(ctx, m, n):
    rng = np.random.default_rng(11)
    Jd = lsq.DeviceMatrix(ctx, lsq.synthetic.dense_inputs(m, n, 5).reshape((m, n), order="F"))
    sv = lsq.AllocatedSolver(Jd, lsq.QR(), for_lm=False)
    return Jd, sv, lsq.DeviceVector(ctx, m, rng.standard_normal(m))


def bench(ctx, tag, m, n, reps, warmup=3):
    L = lsq.lib()
    Jd, sv, dy = dense_setup(ctx, m, n)
    dx = lsq.DeviceVector(ctx, n)
    dq, dse, dt, dck = [lsq.DeviceVector(ctx, m) for _ in range(4)]
    s2 = C.c_double(0.0)
    calls = {
        "solve": lambda: sv.ldiv_(dx, dy),
        "leverage": lambda: lsq._lib.check(L.lsq_dense_qr_leverage(sv.h, Jd.h, None, 0, 0, None, dq.ptr, None, None, None, None, None)),
        "leverage_all": lambda: lsq._lib.check(L.lsq_dense_qr_leverage(sv.h, Jd.h, None, 0, 0, dy.ptr, dq.ptr, dse.ptr, dt.ptr,
                                                                       dck.ptr, C.byref(s2), None)),
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
    out = {"bench": "dense_qr_leverage", "size": tag, "m": m, "n": n, "reps": reps, "qr_path": paths,
           "flops": {"qr": 2.0 * m * n * n - 2.0 * n ** 3 / 3.0, "product": float(m) * n * n}}
    for k in calls:
        out[k] = {"event_median_s": statistics.median(t[k]), "event_min_s": min(t[k])}
    out["leverage_over_solve"] = out["leverage"]["event_median_s"] / out["solve"]["event_median_s"]
    out["leverage_all_over_solve"] = out["leverage_all"]["event_median_s"] / out["solve"]["event_median_s"]
    out["leverage_minus_solve_s"] = out["leverage"]["event_median_s"] - out["solve"]["event_median_s"]
    out["product_tflops_from_difference"] = out["flops"]["product"] / max(out["leverage_minus_solve_s"], 1e-12) * 1e-12
    print(json.dumps(out), flush=True)
    for o in (sv, Jd):
        o.free()


def kernels(ctx, tag, m, n, calls):
    L = lsq.lib()
    Jd, sv, dy = dense_setup(ctx, m, n)
    dq = lsq.DeviceVector(ctx, m)
    for _ in range(calls):
        lsq._lib.check(L.lsq_dense_qr_leverage(sv.h, Jd.h, None, 0, 0, None, dq.ptr, None, None, None, None, None))
    ctx.sync()
    for o in (sv, Jd):
        o.free()
    B, mb, nb, ng = m // 128, 96, 64, n
    Jb = lsq.DeviceMatrix(ctx, lsq.BorderedBlockDiagonal(B, mb, nb, ng, data=lsq.synthetic.bordered_inputs(B, mb, nb, ng, 5)))
    sb = lsq.AllocatedSolver(Jb, lsq.BorderedQR(), for_lm=True)
    dcross = lsq.DeviceVector(ctx, B * nb * ng)
    for _ in range(calls):
        lsq._lib.check(L.lsq_bordered_qr_covariance(sb.h, Jb.h, None, None, None, dcross.ptr, None))
    ctx.sync()
    print(json.dumps({"bench": "leverage_kernels", "size": tag, "calls": calls,
                      "k_lev_tall": {"rows": m, "n": n, "flops": float(m) * n * n},
                      "k_bqc_tall": {"rows": B * nb, "ng": ng, "flops": 2.0 * B * nb * ng * ng}}), flush=True)
    for o in (sb, Jb):
        o.free()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=[s[0] for s in SIZES])
    ap.add_argument("--kernels", type=int, default=0, metavar="N")
    a = ap.parse_args()
    ctx = lsq.default_context()
    for tag, m, n in SIZES:
        if a.only in (None, tag):
            if a.kernels:
                kernels(ctx, tag, m, n, a.kernels)
            else:
                bench(ctx, tag, m, n, a.reps)
