"""lsq_bordered_qr_leverage (lsq_lev_bordered.hip) on the shapes of tools/bordered_cov_bench.py, one JSON line per shape.

    python tools/bordered_leverage_bench.py [--shapes 4096,64,8,256 512,128,32,1024] [--reps 10] [--only-lev N]

What is reported, per shape (B, mb, nb, ng), in one process on the handle of a synthetic.TanhProblem (bordered=...):
    ldiv_qr          one lsq_ldiv_damped of the same BorderedQR() solver (tools/blockdiag_bench.time_solve: device events and the
                     host clock, median and minimum of `reps` after 3 warm-ups): the yardstick -- a leverage call runs the same
                     elimination and the same inner factorisation.
    lev_q / lev_all  one lsq_bordered_qr_leverage on J's own rows, timed the same way: the leverages alone (no residual), and
                     everything (q, se, t, cook, s2) with a residual; each with its ratio to ldiv_qr.
    flops            2 m nb ng (E = C - Z W_b, k_bl_local) and m ng^2 (the triangular product of k_lev_tall on E), and the time
                     that many flops take at the 78.6 TFLOP/s of the datasheet's fp64 matrix rate.  The kernels' own times are
                     not events here: run `--only-lev N` (N calls asking for everything and nothing else) under the profiler's
                     kernel trace, in a run of its own, and divide the totals of k_bl_local and k_lev_tall by N.
    traffic          the bound behind the elimination: J_b and C read once, E written once and read once, at 6.3 TB/s and at the
                     8 TB/s of the datasheet; beside it what the kernels move as written: k_lev_tall stages the slab of E once
                     per tile column of X_g (ceil(ng / 64) (ceil(ng / 64) + 1) / 2 k-tiles of 64 for ceil(ng / 64) of E).
Nothing here is a gate."""
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
from blockdiag_bench import ACHIEVABLE_TBS, PEAK_TBS, HipEvents, time_solve  # noqa: E402

FP64_MATRIX_TFLOPS = 78.6


def call(sv, Jd, df, outs, s2):
    ptr = lambda d: d.ptr if d is not None else None
    return lsq.lib().lsq_bordered_qr_leverage(sv.h, Jd.h, 0, None, 0, None, 0, 0, ptr(df), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]),
                                              ptr(outs[3]), C.byref(s2) if df is not None else None, None)


def time_lev(ctx, sv, Jd, df, outs, reps, warmup=3):
    """outs: (d_q, d_se, d_student, d_cook) DeviceVectors or None."""
    evs = HipEvents(ctx)
    s2 = C.c_double(0.0)
    ev, wall = [], []
    for k in range(warmup + reps):
        ctx.sync()
        t0 = time.perf_counter()
        evs.start()
        rc = call(sv, Jd, df, outs, s2)
        sec = evs.stop()
        t1 = time.perf_counter()
        assert rc == 0, lsq.lib().lsq_last_error().decode()
        if k >= warmup:
            ev.append(sec)
            wall.append(t1 - t0)
    return {"event_median_s": statistics.median(ev), "event_min_s": min(ev), "wall_median_s": statistics.median(wall),
            "wall_min_s": min(wall), "reps": reps}


def traffic_bytes(B, mb, nb, ng):
    """(the bound, what k_bl_local and k_lev_tall move as written), bytes."""
    m = B * mb
    tiles = -(-ng // 64)
    e = 8.0 * m * ng
    bound = 8.0 * m * nb + 3.0 * e                       # J_b, C | E written, E read
    slabs = B * -(-mb // 64)
    local = 8.0 * m * nb + 2.0 * e + 8.0 * slabs * (nb * nb + nb * ng)      # ... and R_b, W_b once per slab
    tall = e * (tiles + 1) / 2.0 + 8.0 * -(-m // 64) * ng * ng / 2.0        # E per k-tile of each tile column | X_g per slab
    return bound, local + tall


def bench_shape(ctx, B, mb, nb, ng, reps, only_lev):
    m, n = B * mb, B * nb + ng
    pr = lsq.synthetic.TanhProblem(m, n, seed=4, ctx=ctx, bordered=(B, mb, nb, ng))
    Jd = lsq.DeviceMatrix(ctx, lsq.BorderedBlockDiagonal(B, mb, nb, ng, data=pr.A))
    rng = np.random.default_rng(5)
    dy = lsq.DeviceVector(ctx, m, rng.standard_normal(m))
    out = {"bench": "bordered_leverage", "B": B, "mb": mb, "nb": nb, "ng": ng, "m": m, "n": n}
    sv = lsq.AllocatedSolver(Jd, lsq.BorderedQR(), for_lm=True)
    outs = tuple(lsq.DeviceVector(ctx, m) for _ in range(4))
    if only_lev:
        s2 = C.c_double(0.0)
        for _ in range(only_lev):
            assert call(sv, Jd, dy, outs, s2) == 0
        ctx.sync()
        out.update(only_lev=only_lev, qr_path=sv.info()["qr_path"], qr_panel=sv.info()["qr_panel"])
        print(json.dumps(out), flush=True)
        pr.close()
        return
    dx = lsq.DeviceVector(ctx, n)
    out["ldiv_qr"] = time_solve(ctx, sv, dx, dy, lsq.DeviceVector(ctx, n, 0.05 + rng.random(n)), reps)
    base = out["ldiv_qr"]["event_median_s"]
    for name, df, o in (("lev_q", None, (outs[0], None, None, None)), ("lev_all", dy, outs)):
        out[name] = time_lev(ctx, sv, Jd, df, o, reps)
        out[name]["over_ldiv_qr"] = out[name]["event_median_s"] / base
    out["qr_path"], out["qr_panel"] = sv.info()["qr_path"], sv.info()["qr_panel"]
    f_local, f_tall = 2.0 * m * nb * ng, 1.0 * m * ng * ng
    out["flops"] = {"local": f_local, "tall": f_tall,
                    "s_at_%.1fTFLOPs" % FP64_MATRIX_TFLOPS: (f_local + f_tall) / (FP64_MATRIX_TFLOPS * 1e12),
                    "workgroups_local": B * -(-mb // 64), "workgroups_tall": -(-m // 64)}
    bound, moved = traffic_bytes(B, mb, nb, ng)
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
    ap.add_argument("--only-lev", type=int, default=0)
    a = ap.parse_args()
    ctx = lsq.default_context()
    for s in a.shapes:
        B, mb, nb, ng = (int(v) for v in s.split(","))
        bench_shape(ctx, B, mb, nb, ng, a.reps, a.only_lev)


if __name__ == "__main__":
    main()
