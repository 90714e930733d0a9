"""lsq_bordered_qr_covariance (lsq_cov_bordered.hip) on the shapes of tools/bordered_qr_bench.py, one JSON line per shape.

    python tools/bordered_cov_bench.py [--shapes 4096,64,8,256 512,128,32,1024] [--reps 10] [--only-cov N]

What is reported, per shape (B, mb, nb, ng), in one process on the handle of a synthetic.TanhProblem (bordered=...):
    ldiv_qr                  one lsq_ldiv_damped of the same BorderedQR() solver (tools/blockdiag_bench.time_solve: device events
                             and the host clock, median and minimum of `reps` after 3 warm-ups): the yardstick -- a covariance
                             runs the same elimination and the same inner factorisation.
    cov_stderr / cov_all / cov_cross_only
                             one lsq_bordered_qr_covariance with a residual, timed the same way, asking for the standard errors
                             alone, for everything (d_cov, d_stderr, d_cross), and for d_cross alone (no per-block kernel);
                             each with its ratio to ldiv_qr.
    tall_product             P = T Cgg: 2 (B nb) ng^2 flops, and the time that many flops take at the 78.6 TFLOP/s of the
                             datasheet's fp64 matrix rate.  The kernel's own time is not an event here: run `--only-cov N` (N
                             covariances asking for everything and nothing else) under the profiler's kernel trace, in a run of
                             its own, and divide k_bqc_tall's total by N.
    traffic                  bytes of T and P as the kernels move them: k_bqc_tsolve reads and writes W once; k_bqc_tall reads T
                             once per tile column of 64 (ceil(ng / 64) times) and Cgg once per row tile, writes P once and
                             d_cross once; k_bqc_block reads T and P once.  Beside it the bound (T read once, P written once,
                             d_cross written once) at 6.3 TB/s and at the 8 TB/s of the datasheet.
Nothing here is a gate."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lsq_amd as lsq  # noqa: E402
from blockdiag_bench import ACHIEVABLE_TBS, PEAK_TBS, HipEvents, time_solve  # noqa: E402

FP64_MATRIX_TFLOPS = 78.6


def time_cov(ctx, sv, Jd, df, outs, reps, warmup=3):
    """outs: (d_cov, d_stderr, d_cross) DeviceVectors or None."""
    evs = HipEvents(ctx)
    ptr = lambda d: d.ptr if d is not None else None
    L = lsq.lib()
    ev, wall = [], []
    for k in range(warmup + reps):
        ctx.sync()
        t0 = time.perf_counter()
        evs.start()
        rc = L.lsq_bordered_qr_covariance(sv.h, Jd.h, df.ptr, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), None)
        sec = evs.stop()
        t1 = time.perf_counter()
        assert rc == 0, L.lsq_last_error().decode()
        if k >= warmup:
            ev.append(sec)
            wall.append(t1 - t0)
    return {"event_median_s": statistics.median(ev), "event_min_s": min(ev), "wall_median_s": statistics.median(wall),
            "wall_min_s": min(wall), "reps": reps}


def traffic_bytes(B, nb, ng):
    """(the bound, what the kernels move as written), bytes, for a call that asks for everything."""
    nr = B * nb
    tiles_c, tiles_r = -(-ng // 64), -(-nr // 64)
    panel = 8.0 * nr * ng
    bound = 3.0 * panel
    tsolve = 2.0 * panel + 8.0 * B * nb * nb * tiles_c
    tall = tiles_c * panel + 8.0 * tiles_r * ng * ng + 2.0 * panel
    block = 2.0 * panel + 8.0 * B * nb * nb * 2
    return bound, tsolve + tall + block


def bench_shape(ctx, B, mb, nb, ng, reps, only_cov):
    m, n = B * mb, B * nb + ng
    pr = lsq.synthetic.TanhProblem(m, n, seed=4, ctx=ctx, bordered=(B, mb, nb, ng))
    Jd = lsq.DeviceMatrix(ctx, lsq.BorderedBlockDiagonal(B, mb, nb, ng, data=pr.A))
    rng = np.random.default_rng(5)
    dy = lsq.DeviceVector(ctx, m, rng.standard_normal(m))
    out = {"bench": "bordered_cov", "B": B, "mb": mb, "nb": nb, "ng": ng, "m": m, "n": n}
    sv = lsq.AllocatedSolver(Jd, lsq.BorderedQR(), for_lm=True)
    dcov, dse, dcr = lsq.DeviceVector(ctx, B * nb * nb + ng * ng), lsq.DeviceVector(ctx, n), lsq.DeviceVector(ctx, B * nb * ng)
    if only_cov:
        for _ in range(only_cov):
            assert lsq.lib().lsq_bordered_qr_covariance(sv.h, Jd.h, dy.ptr, dcov.ptr, dse.ptr, dcr.ptr, None) == 0
        ctx.sync()
        out.update(only_cov=only_cov, qr_path=sv.info()["qr_path"], qr_panel=sv.info()["qr_panel"])
        print(json.dumps(out), flush=True)
        pr.close()
        return
    dx = lsq.DeviceVector(ctx, n)
    out["ldiv_qr"] = time_solve(ctx, sv, dx, dy, lsq.DeviceVector(ctx, n, 0.05 + rng.random(n)), reps)
    base = out["ldiv_qr"]["event_median_s"]
    for name, outs in (("cov_stderr", (None, dse, None)), ("cov_all", (dcov, dse, dcr)), ("cov_cross_only", (None, None, dcr))):
        out[name] = time_cov(ctx, sv, Jd, dy, outs, reps)
        out[name]["over_ldiv_qr"] = out[name]["event_median_s"] / base
    out["qr_path"], out["qr_panel"] = sv.info()["qr_path"], sv.info()["qr_panel"]
    flops = 2.0 * B * nb * ng * ng
    out["tall_product"] = {"flops": flops, "s_at_%.1fTFLOPs" % FP64_MATRIX_TFLOPS: flops / (FP64_MATRIX_TFLOPS * 1e12),
                           "workgroups": -(-(B * nb) // 64) * -(-ng // 64)}
    bound, moved = traffic_bytes(B, nb, ng)
    out["traffic"] = {"bound_bytes": bound, "moved_bytes": moved,
                      "bound_s_at_%.1fTBs" % ACHIEVABLE_TBS: bound / (ACHIEVABLE_TBS * 1e12),
                      "bound_s_at_%.1fTBs" % PEAK_TBS: bound / (PEAK_TBS * 1e12),
                      "moved_s_at_%.1fTBs" % ACHIEVABLE_TBS: moved / (ACHIEVABLE_TBS * 1e12)}
    print(json.dumps(out), flush=True)
    sv.free()
    Jd.free()
    pr.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["4096,64,8,256", "512,128,32,1024"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only-cov", type=int, default=0)
    a = ap.parse_args()
    ctx = lsq.default_context()
    for s in a.shapes:
        B, mb, nb, ng = (int(v) for v in s.split(","))
        bench_shape(ctx, B, mb, nb, ng, a.reps, a.only_cov)


if __name__ == "__main__":
    main()
