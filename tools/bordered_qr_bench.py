"""BorderedQR() on a bordered block-diagonal handle (lsq_borderedqr.hip) against Schur() and LSMR() on the same handle, one JSON
line per shape: the shapes and the protocol of tools/bordered_schur_bench.py.

    python tools/bordered_qr_bench.py [--shapes 4096,64,8,256 512,128,32,1024] [--reps 10] [--only-solve N]

What is timed, per shape (B, mb, nb, ng), in one process on the handle of a synthetic.TanhProblem (bordered=...; f! and g! on the
device, no host callbacks):
    ldiv_qr / ldiv_schur / ldiv_lsmr
                             one lsq_ldiv_damped on the generator's values, y standard normal, damping 0.05 + U(0,1): device events
                             and the host clock around the call (which ends in a read of the status words / a drained stream),
                             median and minimum of `reps` after 3 warm-ups.  LSMR() at its default tolerances.  The distance of
                             Schur()'s and LSMR()'s x from BorderedQR()'s is reported.
    lm_qr / lm_schur / lm_lsmr
                             a whole LevenbergMarquardt fit from x0 = 0 with the default tolerances each way (lsq_result.seconds,
                             median of `reps` after 2 warm-ups), with outer / inner iteration counts and the final ssr.
    eliminate_traffic        the bound of the elimination: one read of the values, one write of the transformed border F and the
                             one read of it by the inner QR(), at 6.3 TB/s (the rate the project's streaming kernels reach) and
                             at the 8 TB/s of the datasheet; and beside it what k_bdq_factor + k_bdq_apply move as written: the
                             reflector scratch (the size of the block values) written once and read once per tile of 64 border
                             columns, R, z, W, r and the taus.  The kernels' own times are not events here: run `--only-solve N`
                             (N BorderedQR() solves and nothing else) under the profiler's kernel trace, in a run of its own, and
                             divide.
Nothing here is a gate."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lsq_amd as lsq  # noqa: E402
from blockdiag_bench import ACHIEVABLE_TBS, PEAK_TBS, time_solve  # noqa: E402


def eliminate_bytes(B, mb, nb, ng):
    """(the bound, what the two kernels move as written), bytes."""
    m = B * mb
    H = 64 if mb > 32 else 32
    nch, ntile = -(-mb // H), -(-ng // 64)
    bound = 8.0 * (m * (nb + ng) + 2 * m * ng)
    factor = 8.0 * (m * nb + m + B * nb) + 8.0 * (m * nb + B * nch * nb + B * nb * nb + B * nb + m)
    apply_ = 8.0 * (m * ng + ntile * (m * nb + B * nch * nb)) + 8.0 * (m * ng + B * nb * ng)
    return bound, factor + apply_


def bench_shape(ctx, B, mb, nb, ng, reps, only_solve):
    LM = lsq._lib.LEVENBERG_MARQUARDT
    m, n = B * mb, B * nb + ng
    pr = lsq.synthetic.TanhProblem(m, n, seed=4, ctx=ctx, bordered=(B, mb, nb, ng))
    Jd = lsq.DeviceMatrix(ctx, lsq.BorderedBlockDiagonal(B, mb, nb, ng, data=pr.A))
    rng = np.random.default_rng(5)
    dy = lsq.DeviceVector(ctx, m, rng.standard_normal(m))
    damp = 0.05 + rng.random(n)
    out = {"bench": "bordered_qr", "B": B, "mb": mb, "nb": nb, "ng": ng, "m": m, "n": n, "nnz": m * (nb + ng)}
    sv = lsq.AllocatedSolver(Jd, lsq.BorderedQR(), for_lm=True)
    dxq = lsq.DeviceVector(ctx, n)
    if only_solve:
        dd = lsq.DeviceVector(ctx, n, damp)
        for _ in range(only_solve):
            sv.ldiv_(dxq, dy, dd)
        ctx.sync()
        out.update(only_solve=only_solve, qr_path=sv.info()["qr_path"], qr_panel=sv.info()["qr_panel"])
        print(json.dumps(out), flush=True)
        pr.close()
        return
    out["ldiv_qr"] = time_solve(ctx, sv, dxq, dy, lsq.DeviceVector(ctx, n, damp), reps)
    out["ldiv_qr"].update(qr_path=sv.info()["qr_path"], qr_panel=sv.info()["qr_panel"])
    xq = dxq.get()
    sv.free()
    ss = lsq.AllocatedSolver(Jd, lsq.Schur(), for_lm=True)
    dxs = lsq.DeviceVector(ctx, n)
    out["ldiv_schur"] = time_solve(ctx, ss, dxs, dy, lsq.DeviceVector(ctx, n, damp), reps)
    out["ldiv_schur"]["rel_distance_from_qr"] = float(np.linalg.norm(dxs.get() - xq) / np.linalg.norm(xq))
    ss.free()
    sl = lsq.AllocatedSolver(Jd, lsq.LSMR(), for_lm=True)
    dxl = lsq.DeviceVector(ctx, n)
    ddl, dd0 = lsq.DeviceVector(ctx, n, damp), lsq.DeviceVector(ctx, n, damp)

    class Fresh:                       # LSMR() leaves sqrt(damp) behind: every timed solve starts from the damping itself
        def ldiv_(self, x, y, d):      # (a device-to-device copy of n doubles in stream order)
            lsq._lib.check(lsq.lib().lsq_d2d(ctx.h, d.ptr, dd0.ptr, 8 * n))
            return sl.ldiv_(x, y, d)

    out["ldiv_lsmr"] = time_solve(ctx, Fresh(), dxl, dy, ddl, reps)
    out["ldiv_lsmr"]["iterations"] = sl.info()["lsmr_iter"]
    out["ldiv_lsmr"]["rel_distance_from_qr"] = float(np.linalg.norm(dxl.get() - xq) / np.linalg.norm(xq))
    out["ldiv_qr_over_schur"] = out["ldiv_qr"]["event_median_s"] / out["ldiv_schur"]["event_median_s"]
    out["ldiv_qr_over_lsmr"] = out["ldiv_qr"]["event_median_s"] / out["ldiv_lsmr"]["event_median_s"]
    sl.free()
    Jd.free()
    bound, moved = eliminate_bytes(B, mb, nb, ng)
    out["eliminate_traffic"] = {"bound_bytes": bound, "moved_bytes": moved,
                                "bound_s_at_%.1fTBs" % ACHIEVABLE_TBS: bound / (ACHIEVABLE_TBS * 1e12),
                                "bound_s_at_%.1fTBs" % PEAK_TBS: bound / (PEAK_TBS * 1e12),
                                "moved_s_at_%.1fTBs" % ACHIEVABLE_TBS: moved / (ACHIEVABLE_TBS * 1e12)}
    for name, kind in (("lm_qr", lsq._lib.BORDERED_QR), ("lm_schur", lsq._lib.SCHUR), ("lm_lsmr", lsq._lib.LSMR)):
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
    out["lm_qr_over_schur"] = out["lm_qr"]["seconds_median"] / out["lm_schur"]["seconds_median"]
    out["lm_qr_over_lsmr"] = out["lm_qr"]["seconds_median"] / out["lm_lsmr"]["seconds_median"]
    print(json.dumps(out), flush=True)
    pr.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["4096,64,8,256", "512,128,32,1024"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only-solve", type=int, default=0)
    a = ap.parse_args()
    ctx = lsq.default_context()
    for s in a.shapes:
        B, mb, nb, ng = (int(v) for v in s.split(","))
        bench_shape(ctx, B, mb, nb, ng, a.reps, a.only_solve)


if __name__ == "__main__":
    main()
