"""Measurements of Cholesky() and BlockQR() on block-diagonal Jacobians (lsq_blockdiag.hip, lsq_blockqr.hip); one JSON line per run.

    python tools/blockdiag_bench.py dense      block solve vs the dense handle's Cholesky() on the stacked matrix
                                               (B=32, mb=512, nb=64: 16384 x 2048, the C3 shape)
    python tools/blockdiag_bench.py roofline   solve time vs 8 B mb (nb+1) bytes at 8 TB/s (peak) and 6.3 TB/s (achievable):
                                               B=8192, mb=256, nb=32 (537 MB of values: past the 256 MiB Infinity Cache) and
                                               B=65536, mb=64, nb=8
    python tools/blockdiag_bench.py lm         LM(Cholesky()) on the block handle vs LM(LSMR()) on a plain CSC handle of the
                                               same matrix (B=8192, mb=256, nb=32): seconds per outer iteration, to convergence
    python tools/blockdiag_bench.py qr         one BlockQR() solve (lsq_blockqr.hip), damped and undamped, against Cholesky() on
                                               the same handle and the HBM floor 8 B mb (nb+1) bytes: B=4096 with 256 x 16,
                                               128 x 32 and 64 x 64 blocks; and against the dense handle's QR() on 16 blocks of
                                               128 x 32 stacked to 2048 x 512
    python tools/blockdiag_bench.py bordered   Cholesky() on a BORDERED block-diagonal handle (lsq_bordered.hip): B=4096, mb=256 with
                                               (nb, ng) = (8, 8) and (32, 16) -- one lsq_ldiv_damped against the HBM floor
                                               8 B mb (nb+ng+1) bytes at 6.3 TB/s, and LM to convergence on the device tanh model
                                               against LevenbergMarquardt(LSMR()) on the same handle (the only way to solve the
                                               problem on the device without this solver)
    python tools/blockdiag_bench.py cov        lsq_solver_covariance (lsq_cov.hip, lsq_bordered.hip): B=4096, mb=256, nb = 16, 32, 64
                                               and bordered (nb, ng) = (8, 8), (32, 16) -- median of 20 after 3 warm-ups, against
                                               Cholesky()'s lsq_ldiv_damped on the same handle in the same run and against the
                                               HBM floor 8 B mb (nb+ng) read + 8 (B nb^2 + ng^2) written at 6.3 TB/s
    python tools/blockdiag_bench.py all        (dense, roofline, lm, qr)
    python tools/blockdiag_bench.py lm --batched   one trust region per block (lsq_optimize_batched) against the stacked loop on
                                               the heterogeneous tanh problem (block b starts from 0.3 (b mod 4) (+1, -1, ..),
                                               0.1 N(0,1) added to the right-hand side of blocks b mod 8 == 5), device model,
                                               B=4096 with 256 x 16 and 128 x 32 blocks: seconds to convergence of each loop
                                               by its own criterion (stacked: the summed one; batched: every block) and
                                               seconds per outer iteration over 10 iterations with zero tolerances (every
                                               block active in both loops)

Every solve is timed with HIP events on the library's stream (hipEventRecord through ctypes) around the whole lsq_ldiv_damped
call -- it ends with the status hand-over to the host, so event time and wall time agree to a few microseconds; both are
reported.  >= 10 timed repeats after 3 warm-up calls, median and min.  Operands: the library's N(0,1)/sqrt(mb) generator."""
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

PEAK_TBS, ACHIEVABLE_TBS = 8.0, 6.3


class HipEvents:
    """hipEvent pairs on the library's stream, through the HIP runtime the library itself is linked against."""

    def __init__(self, ctx):
        self.hip = C.CDLL("libamdhip64.so")
        lsq.lib().lsq_ctx_stream.restype = C.c_void_p
        self.stream = C.c_void_p(lsq.lib().lsq_ctx_stream(ctx.h))
        self.e0, self.e1 = C.c_void_p(), C.c_void_p()
        for e in (self.e0, self.e1):
            assert self.hip.hipEventCreate(C.byref(e)) == 0

    def start(self):
        assert self.hip.hipEventRecord(self.e0, self.stream) == 0

    def stop(self):
        assert self.hip.hipEventRecord(self.e1, self.stream) == 0
        assert self.hip.hipEventSynchronize(self.e1) == 0
        ms = C.c_float(0.0)
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.e0, self.e1) == 0
        return ms.value * 1e-3


def time_solve(ctx, sv, dx, dy, dd, reps, warmup=3):
    evs = HipEvents(ctx)
    ev, wall = [], []
    for k in range(warmup + reps):
        ctx.sync()
        t0 = time.perf_counter()
        evs.start()
        sv.ldiv_(dx, dy, dd)
        sec = evs.stop()
        t1 = time.perf_counter()
        if k >= warmup:
            ev.append(sec)
            wall.append(t1 - t0)
    return {"event_median_s": statistics.median(ev), "event_min_s": min(ev), "wall_median_s": statistics.median(wall),
            "wall_min_s": min(wall), "reps": reps}


def block_operands(ctx, B, mb, nb, seed):
    J = lsq.BlockDiagonal(B, mb, nb, data=lsq.synthetic.blockdiag_inputs(B, mb, nb, seed))
    rng = np.random.default_rng(seed)
    y = rng.standard_normal(B * mb)
    damp = 0.05 + rng.random(B * nb)
    return J, y, damp


def bench_dense(ctx, reps):
    B, mb, nb = 32, 512, 64
    J, y, damp = block_operands(ctx, B, mb, nb, 1)
    out = {"bench": "block_vs_dense", "B": B, "mb": mb, "nb": nb}
    xs = {}
    for name, host in (("block", J), ("dense", J.toarray())):
        Jd = lsq.DeviceMatrix(ctx, host)
        sv = lsq.AllocatedSolver(Jd, lsq.Cholesky(), for_lm=True)
        dx, dy, dd = lsq.DeviceVector(ctx, Jd.n), lsq.DeviceVector(ctx, Jd.m, y), lsq.DeviceVector(ctx, Jd.n, damp)
        out[name] = time_solve(ctx, sv, dx, dy, dd, reps)
        out[name]["path"] = sv.info()["blockdiag_path"] or sv.info()["chol_path"]
        xs[name] = dx.get()
    out["rel_diff"] = float(np.linalg.norm(xs["block"] - xs["dense"]) / np.linalg.norm(xs["dense"]))
    out["speedup_event_median"] = out["dense"]["event_median_s"] / out["block"]["event_median_s"]
    print(json.dumps(out))


def bench_roofline(ctx, reps):
    for B, mb, nb in ((8192, 256, 32), (65536, 64, 8)):
        J, y, damp = block_operands(ctx, B, mb, nb, 2)
        Jd = lsq.DeviceMatrix(ctx, J)
        sv = lsq.AllocatedSolver(Jd, lsq.Cholesky(), for_lm=True)
        dx, dy, dd = lsq.DeviceVector(ctx, Jd.n), lsq.DeviceVector(ctx, Jd.m, y), lsq.DeviceVector(ctx, Jd.n, damp)
        t = time_solve(ctx, sv, dx, dy, dd, reps)
        nbytes = 8.0 * B * mb * (nb + 1) + 16.0 * B * nb
        out = {"bench": "roofline", "B": B, "mb": mb, "nb": nb, "bytes": nbytes, **t}
        out["tb_per_s_event_median"] = nbytes / t["event_median_s"] * 1e-12
        out["fraction_of_peak_8TBs"] = out["tb_per_s_event_median"] / PEAK_TBS
        out["fraction_of_achievable_6.3TBs"] = out["tb_per_s_event_median"] / ACHIEVABLE_TBS
        print(json.dumps(out))
        Jd.free()


def bench_qr(ctx, reps):
    for B, mb, nb in ((4096, 256, 16), (4096, 128, 32), (4096, 64, 64)):
        J, y, damp = block_operands(ctx, B, mb, nb, 3)
        Jd = lsq.DeviceMatrix(ctx, J)
        dx, dy, dd = lsq.DeviceVector(ctx, Jd.n), lsq.DeviceVector(ctx, Jd.m, y), lsq.DeviceVector(ctx, Jd.n, damp)
        floor_bytes = 8.0 * B * mb * (nb + 1)
        out = {"bench": "blockqr_vs_cholesky", "B": B, "mb": mb, "nb": nb, "floor_bytes": floor_bytes,
               "floor_s_at_6.3TBs": floor_bytes / (ACHIEVABLE_TBS * 1e12)}
        xs = {}
        for name, solver in (("blockqr", lsq.BlockQR()), ("cholesky", lsq.Cholesky())):
            for leg, d in (("damped", dd), ("undamped", None)):
                sv = lsq.AllocatedSolver(Jd, solver, for_lm=d is not None)
                out[name + "_" + leg] = time_solve(ctx, sv, dx, dy, d, reps)
                xs[name + "_" + leg] = dx.get()
        for leg in ("damped", "undamped"):
            out["rel_diff_" + leg] = float(np.linalg.norm(xs["blockqr_" + leg] - xs["cholesky_" + leg]) /
                                           np.linalg.norm(xs["cholesky_" + leg]))
            out["qr_over_cholesky_" + leg] = out["blockqr_" + leg]["event_median_s"] / out["cholesky_" + leg]["event_median_s"]
            out["qr_over_floor_" + leg] = out["blockqr_" + leg]["event_median_s"] / out["floor_s_at_6.3TBs"]
        print(json.dumps(out))
        Jd.free()
    B, mb, nb = 16, 128, 32
    J, y, damp = block_operands(ctx, B, mb, nb, 3)
    out = {"bench": "blockqr_vs_dense_qr", "B": B, "mb": mb, "nb": nb}
    xs = {}
    for name, host, solver in (("blockqr", J, lsq.BlockQR()), ("dense_qr", J.toarray(), lsq.QR())):
        Jd = lsq.DeviceMatrix(ctx, host)
        dx, dy = lsq.DeviceVector(ctx, Jd.n), lsq.DeviceVector(ctx, Jd.m, y)
        sv = lsq.AllocatedSolver(Jd, solver, for_lm=False)
        out[name] = time_solve(ctx, sv, dx, dy, None, reps)
        xs[name] = dx.get()
    out["rel_diff"] = float(np.linalg.norm(xs["blockqr"] - xs["dense_qr"]) / np.linalg.norm(xs["dense_qr"]))
    out["speedup_event_median"] = out["dense_qr"]["event_median_s"] / out["blockqr"]["event_median_s"]
    print(json.dumps(out))


def bench_lm(ctx, reps):
    B, mb, nb = 8192, 256, 32
    m, n = B * mb, B * nb
    out = {"bench": "lm_cholesky_vs_lsmr", "B": B, "mb": mb, "nb": nb}
    pr = lsq.synthetic.TanhProblem(m, n, seed=4, ctx=ctx, blockdiag=(B, mb, nb))
    A, b = pr.A, pr.b
    S = lsq.BlockDiagonal(B, mb, nb, data=A).tocsc()
    pl = lsq.synthetic.TanhProblem(m, n, sparse=True, seed=4, ctx=ctx, b=b,
                                   inputs=(S.indptr.astype(np.int32), S.indices.astype(np.int32), A))
    for name, p, kind in (("cholesky_block", pr, lsq._lib.CHOLESKY), ("lsmr_csc", pl, lsq._lib.LSMR)):
        runs = []
        for k in range(2 + reps):
            p.reset()
            r = p.optimize(lsq._lib.LEVENBERG_MARQUARDT, kind, iterations=50, fetch_x=False)
            if k >= 2:
                runs.append(r)
        sec = [r.seconds for r in runs]
        r = runs[-1]
        out[name] = {"converged": r.converged, "outer_iterations": r.iterations, "lsmr_inner_iterations": r.lsmr_iterations,
                     "ssr": r.ssr, "seconds_median": statistics.median(sec), "seconds_min": min(sec),
                     "seconds_per_outer_median": statistics.median(sec) / max(r.iterations, 1), "reps": reps}
    out["speedup_to_convergence"] = out["lsmr_csc"]["seconds_median"] / out["cholesky_block"]["seconds_median"]
    print(json.dumps(out))
    pr.close()
    pl.close()


def bench_bordered(ctx, reps):
    LM = lsq._lib.LEVENBERG_MARQUARDT
    for nb, ng in ((8, 8), (32, 16)):
        B, mb = 4096, 256
        m, n = B * mb, B * nb + ng
        pr = lsq.synthetic.TanhProblem(m, n, seed=4, ctx=ctx, bordered=(B, mb, nb, ng))
        floor_bytes = 8.0 * B * mb * (nb + ng + 1)
        out = {"bench": "bordered_cholesky", "B": B, "mb": mb, "nb": nb, "ng": ng, "floor_bytes": floor_bytes,
               "floor_s_at_6.3TBs": floor_bytes / (ACHIEVABLE_TBS * 1e12)}
        Jd = lsq.DeviceMatrix(ctx, lsq.BorderedBlockDiagonal(B, mb, nb, ng, data=pr.A))
        rng = np.random.default_rng(5)
        sv = lsq.AllocatedSolver(Jd, lsq.Cholesky(), for_lm=True)
        dx, dy = lsq.DeviceVector(ctx, n), lsq.DeviceVector(ctx, m, rng.standard_normal(m))
        dd = lsq.DeviceVector(ctx, n, 0.05 + rng.random(n))
        out["ldiv_damped"] = time_solve(ctx, sv, dx, dy, dd, reps)
        out["ldiv_damped_over_floor"] = out["ldiv_damped"]["event_median_s"] / out["floor_s_at_6.3TBs"]
        sv.free()
        Jd.free()
        for name, kind in (("lm_cholesky", lsq._lib.CHOLESKY), ("lm_lsmr", lsq._lib.LSMR)):
            runs = []
            for k in range(2 + reps):
                pr.reset()
                r = pr.optimize(LM, kind, iterations=50, fetch_x=False)
                if k >= 2:
                    runs.append(r)
            sec = [r.seconds for r in runs]
            r = runs[-1]
            out[name] = {"converged": r.converged, "outer_iterations": r.iterations, "lsmr_inner_iterations": r.lsmr_iterations,
                         "ssr": r.ssr, "seconds_median": statistics.median(sec), "seconds_min": min(sec),
                         "seconds_per_outer_median": statistics.median(sec) / max(r.iterations, 1), "reps": reps}
        out["speedup_to_convergence"] = out["lm_lsmr"]["seconds_median"] / out["lm_cholesky"]["seconds_median"]
        print(json.dumps(out), flush=True)
        pr.close()


def bench_batched(ctx, reps):
    LM, CH = lsq._lib.LEVENBERG_MARQUARDT, lsq._lib.CHOLESKY
    for B, mb, nb in ((4096, 256, 16), (4096, 128, 32)):
        m, n = B * mb, B * nb
        A = lsq.synthetic.blockdiag_inputs(B, mb, nb, 4)
        A3 = A.reshape((B, nb, mb))
        _, b = lsq.synthetic.rhs_for(lambda t: np.einsum("bjr,bj->br", A3, t.reshape((B, nb))).reshape(-1), m, n, 4)
        noisy = np.repeat(np.arange(B) % 8 == 5, mb)
        b[noisy] += 0.1 * lsq.synthetic.normal(m, 4 + 303)[noisy]
        x0 = (0.3 * np.repeat(np.arange(B) % 4, nb) * np.tile(np.where(np.arange(nb) % 2 == 0, 1.0, -1.0), B)).astype(np.float64)
        pr = lsq.synthetic.TanhProblem(m, n, ctx=ctx, blockdiag=(B, mb, nb), inputs=A, b=b)
        out = {"bench": "batched_vs_stacked", "B": B, "mb": mb, "nb": nb, "reps": reps}

        def timed(fn):
            runs = []
            for k in range(2 + reps):
                pr.reset(x0)
                ctx.sync()
                r = fn()
                if k >= 2:
                    runs.append(r)
            sec = [r.seconds for r in runs]
            return runs[-1], statistics.median(sec), min(sec), max(sec)

        r, med, lo, hi = timed(lambda: pr.optimize_batched(LM, CH, iterations=200, fetch_x=False))
        out["batched"] = {"all_converged": bool(np.all(r.converged == 1)), "outer_iterations": r.outer_iterations,
                          "iterations_min": int(r.iterations.min()), "iterations_median": float(np.median(r.iterations)),
                          "ssr": float(r.ssr.sum()), "seconds_median": med, "seconds_min": lo, "seconds_max": hi}
        r, med, lo, hi = timed(lambda: pr.optimize(LM, CH, iterations=200, fetch_x=False))
        out["stacked"] = {"converged": r.converged, "outer_iterations": r.iterations, "ssr": r.ssr, "seconds_median": med,
                          "seconds_min": lo, "seconds_max": hi}
        K = 10
        r, med, lo, hi = timed(lambda: pr.optimize_batched(LM, CH, x_tol=0.0, f_tol=0.0, g_tol=0.0, iterations=K, fetch_x=False))
        out["batched"]["us_per_outer_all_active"] = {"median": med / K * 1e6, "min": lo / K * 1e6, "max": hi / K * 1e6}
        r, med, lo, hi = timed(lambda: pr.optimize(LM, CH, x_tol=0.0, f_tol=0.0, g_tol=0.0, iterations=K, fetch_x=False))
        out["stacked"]["us_per_outer_all_active"] = {"median": med / K * 1e6, "min": lo / K * 1e6, "max": hi / K * 1e6}
        print(json.dumps(out))
        pr.close()


def time_call(ctx, fn, reps, warmup=3):
    evs = HipEvents(ctx)
    ev = []
    for k in range(warmup + reps):
        ctx.sync()
        evs.start()
        fn()
        sec = evs.stop()
        if k >= warmup:
            ev.append(sec)
    return {"event_median_s": statistics.median(ev), "event_min_s": min(ev), "reps": reps}


def bench_cov(ctx, reps):
    """lsq_solver_covariance against Cholesky()'s lsq_ldiv_damped on the same handle in the same run, and against the HBM floor
    (values read once, covariance written once) at 6.3 TB/s.  Outputs stay on the device (the C entry point, no download)."""
    B, mb = 4096, 256
    L = lsq.lib()
    for nb, ng in ((16, 0), (32, 0), (64, 0), (8, 8), (32, 16)):
        m, n = B * mb, B * nb + ng
        if ng:
            J = lsq.BorderedBlockDiagonal(B, mb, nb, ng, data=lsq.synthetic.bordered_inputs(B, mb, nb, ng, 6))
        else:
            J = lsq.BlockDiagonal(B, mb, nb, data=lsq.synthetic.blockdiag_inputs(B, mb, nb, 6))
        floor_bytes = 8.0 * B * mb * (nb + ng) + 8.0 * (B * nb * nb + ng * ng)
        out = {"bench": "covariance", "B": B, "mb": mb, "nb": nb, "ng": ng, "floor_bytes": floor_bytes,
               "floor_s_at_6.3TBs": floor_bytes / (ACHIEVABLE_TBS * 1e12)}
        Jd = lsq.DeviceMatrix(ctx, J)
        rng = np.random.default_rng(7)
        sv = lsq.AllocatedSolver(Jd, lsq.Cholesky(), for_lm=True)
        dx, dy = lsq.DeviceVector(ctx, n), lsq.DeviceVector(ctx, m, rng.standard_normal(m))
        dd = lsq.DeviceVector(ctx, n, 0.05 + rng.random(n))
        dcov, dse = lsq.DeviceVector(ctx, B * nb * nb + ng * ng), lsq.DeviceVector(ctx, n)
        out["ldiv_damped"] = time_solve(ctx, sv, dx, dy, dd, reps)
        for name, f in (("covariance", None), ("covariance_with_f", dy.ptr)):
            out[name] = time_call(ctx, lambda: lsq._lib.check(L.lsq_solver_covariance(sv.h, Jd.h, f, dcov.ptr, dse.ptr, None)), reps)
            out[name + "_over_ldiv_damped"] = out[name]["event_median_s"] / out["ldiv_damped"]["event_median_s"]
            out[name + "_over_floor"] = out[name]["event_median_s"] / out["floor_s_at_6.3TBs"]
        print(json.dumps(out))
        sv.free()
        Jd.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["dense", "roofline", "lm", "qr", "bordered", "cov", "all"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batched", action="store_true", help="the per-block trust-region loop against the stacked one (only this leg)")
    a = ap.parse_args()
    ctx = lsq.default_context()
    if a.batched:
        bench_batched(ctx, max(a.reps, 10))
        return
    if a.what == "bordered":
        bench_bordered(ctx, max(a.reps, 10))
        return
    if a.what == "cov":
        bench_cov(ctx, max(a.reps, 10))
        return
    if a.what in ("dense", "all"):
        bench_dense(ctx, max(a.reps, 10))
    if a.what in ("roofline", "all"):
        bench_roofline(ctx, max(a.reps, 10))
    if a.what in ("lm", "all"):
        bench_lm(ctx, max(a.reps, 10))
    if a.what in ("qr", "all"):
        bench_qr(ctx, max(a.reps, 10))


if __name__ == "__main__":
    main()
