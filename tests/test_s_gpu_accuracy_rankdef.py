"""Accuracy tier on the device, rank-deficient part: the five implementations of the reference's pivoted QR solve
(qr!(J, ColumnNorm()) + the rank-revealing minimum-norm ldiv!, dense_qr.jl:37,83) -- k_qrcp_solve; k_qr_norms / k_qr_pivot /
k_qr_apply with k_qr_rank and the completion in k_qrcp_solve; k_qr2_step<1|2|4> + k_qr2_gather; the same one-stage kernels as
the sweep on R beyond n = 2048 (lsq_qr.hip); the two geometries of lsq_blockqr.hip -- on operands whose rank is NOT n, held to
LAPACK's own error.  tests/test_h_gpu_accuracy.py and tests/test_i_gpu_accuracy_dense.py assert qr_rank == n throughout; the
shape tier has rank-deficient operands in one form only (randn(m, r) @ randn(r, n): sixteen decades between sigma_r and
sigma_(r+1), one column scale, no ties, allclose at 1e-8).

Operands, references, metrics and case lists: tests/rankdef_common.py; certified without a device by
tests/test_rankdef_host.py (the oracle alone finds the intended rank on every case; the rule accepts LAPACK's dgelsy and
rejects a solution truncated one rank early, a basic solution without the minimum-norm completion and, for family T, a rank
decided with 100 rcond).
    E   exact rank r, A = (B C) D from integer factors: x_hp = (C D)^+ B^+ y in longdouble, e = ||x - x_hp|| / ||x_hp||,
        e_ref from O.qr_solve, ac.judge with k = n; device rank == oracle rank == r
    T   singular values down to K rcond, then rcond / K: device rank == oracle rank == the intended one; the residual
        rho(x) = ||A x - y|| / (||A||_F ||x|| + ||y||) within 16 max(|rho_orc - rho_hp|, 64 * 2^-53) of the longdouble one.
        Measured on the CPU (tests/test_rankdef_host.py lists every case): |rho_orc - rho_hp| = 5e-18 .. 8e-16, below the
        floor, so the bound is 16 * 64 * 2^-53 = 1.14e-13 -- except 900 x 100, r 37, K 30 (1.7e-14: bound 2.75e-13) and
        2100 x 2049, r 5 (1.6e-14: bound 2.55e-13); rho_hp itself is 1.4e-12 .. 1.4e-9, and a rank decided with 100 rcond moves
        it by 2.4e-13 .. 2.7e-7.  A deficient case must come back as two-stage-pivoted without LSQ_QR_ALWAYS_PIVOT: the
        certificate refused it
    Z   LM's stacked operand with z all-zero columns (damp = 0.1 colsumabs2 is exactly 0 there): rank n - z under
        rcond = n eps, x_j == 0.0 where the oracle's is, damping vector untouched, ac.solve_err over the other columns
Every case asserts info()["qr_path"] and prints its PATH and ACC lines.  Switches are set through monkeypatch only.  The seeds
were fixed before the first device run; no case is skipped, expected to fail or reseeded."""
import numpy as np
import pytest

import accuracy_common as ac
import rankdef_common as rc
from gpu_common import lsq

pytestmark = pytest.mark.gpu


def device_solve(ctx, A, y, damp=None):
    Jd = lsq.DeviceMatrix(ctx, A)
    sv = lsq.AllocatedSolver(Jd, lsq.QR(), for_lm=damp is not None)
    dx = lsq.DeviceVector(ctx, Jd.n)
    dd = lsq.DeviceVector(ctx, Jd.n, damp) if damp is not None else None
    _, nmul = sv.ldiv_(dx, lsq.DeviceVector(ctx, Jd.m, y), dd)
    x, info = dx.get(), sv.info()
    damp_after = dd.get() if dd is not None else None
    sv.free()
    Jd.free()
    assert nmul == 1
    return x, info, damp_after


def setenv(monkeypatch, path):
    for k, v in rc.ENV[path].items():
        monkeypatch.setenv(k, v)


# ------------------------------------------------------------------------------------------ family E
def run_e(ctx, path, m, n, r, variant, want_path):
    ref = rc.e_ref(m, n, r, variant)
    x, info, _ = device_solve(ctx, ref.op.A, ref.op.y)
    what = "%s %dx%d r=%d %s" % (path, m, n, r, variant)
    print("PATH E %s | %s rank %s (oracle %d)" % (what, info["qr_path"], info["qr_rank"], ref.rank_orc))
    assert ref.rank_orc == r, (what, ref.rank_orc)
    assert info["qr_path"] == want_path, (what, info)
    assert info["qr_rank"] == r, (what, info)
    ac.judge("rankdef E " + what, [("x", rc.rel_err(x, ref.x_hp), ref.e_ref, n)])


@pytest.mark.parametrize("path,m,n,r,variant", rc.E_CASES)
def test_exact_rank(ctx, monkeypatch, path, m, n, r, variant):
    setenv(monkeypatch, path)
    run_e(ctx, path, m, n, r, variant, rc.QR_PATH[path])


def test_exact_rank_beyond_2048_columns(ctx, monkeypatch):
    """n = 2049: the two-stage path hands R to k_qr_norms / k_qr_pivot / k_qr_apply (k_qr2_step holds at most 2048 rows), and
    the rank decision and the completion run in k_qrcp_solve (k_qr_rank's LDS ends at 2048)."""
    path, m, n, r, variant = rc.E_SWEEP_CASE
    setenv(monkeypatch, path)
    run_e(ctx, path, m, n, r, variant, rc.QR_PATH[path])


@pytest.mark.parametrize("m,n,r,variant,want_path", rc.E_DEFAULT_CASES)
def test_exact_rank_default_dispatch(ctx, m, n, r, variant, want_path):
    run_e(ctx, "default", m, n, r, variant, want_path)


# ------------------------------------------------------------------------------------------ family T
def run_t(ctx, path, m, n, r, K):
    ref = rc.t_ref(m, n, r, K)
    x, info, _ = device_solve(ctx, ref.A, ref.y)
    what = "%s %dx%d r=%d K=%d" % (path, m, n, r, K)
    print("PATH T %s | %s rank %s (oracle %d)" % (what, info["qr_path"], info["qr_rank"], ref.rank_orc))
    assert ref.rank_orc == r, (what, ref.rank_orc)
    assert info["qr_rank"] == r, (what, info)
    if path in ("two-stage", "sweep") and r == n:          # just full rank: either the certificate proves it or the sweep finds it
        assert info["qr_path"] in ("two-stage-pivoted", "two-stage-certified"), (what, info)
    else:
        assert info["qr_path"] == rc.QR_PATH[path], (what, info)
    ref.judge("rankdef T " + what, x)


@pytest.mark.parametrize("path,m,n,r,K", rc.T_CASES)
def test_rank_near_the_threshold(ctx, monkeypatch, path, m, n, r, K):
    setenv(monkeypatch, path)
    run_t(ctx, path, m, n, r, K)


def test_rank_near_the_threshold_beyond_2048_columns(ctx, monkeypatch):
    path, m, n, r, K = rc.T_SWEEP_CASE
    setenv(monkeypatch, path)
    run_t(ctx, path, m, n, r, K)


# ------------------------------------------------------------------------------------------ family Z
@pytest.mark.parametrize("path,m,n,z,variant", rc.Z_CASES)
def test_stacked_operand_with_zero_columns(ctx, monkeypatch, path, m, n, z, variant):
    for k, v in rc.z_env(path, m, n).items():
        monkeypatch.setenv(k, v)
    ref = rc.z_ref(m, n, z, variant)
    x, info, damp_after = device_solve(ctx, ref.A, ref.y, ref.damp)
    what = "%s %dx%d z=%d %s" % (path, m, n, z, variant)
    print("PATH Z %s | %s rank %s (oracle %d)" % (what, info["qr_path"], info["qr_rank"], ref.rank_orc))
    assert ref.rank_orc == n - z, (what, ref.rank_orc)
    assert info["qr_path"] == rc.QR_PATH[path], (what, info)
    assert info["qr_rank"] == n - z, (what, info)
    assert np.array_equal(damp_after, ref.damp), what
    zero = np.flatnonzero(ref.x_orc == 0.0)
    assert len(zero) == z and np.all(x[zero] == 0.0), (what, x[zero])
    ac.judge("rankdef Z " + what, [("x", ref.err(x), ref.e_ref, n)])


# ------------------------------------------------------------------------------------------ BlockQR()
def bq_solve(ctx, blocks, damp=None):
    J = lsq.BlockDiagonal.from_blocks([np.array(b.A) for b in blocks])
    y = np.concatenate([b.y for b in blocks])
    Jd = lsq.DeviceMatrix(ctx, J)
    sv = lsq.AllocatedSolver(Jd, lsq.BlockQR(), for_lm=damp is not None)
    dx = lsq.DeviceVector(ctx, Jd.n)
    dd = lsq.DeviceVector(ctx, Jd.n, damp) if damp is not None else None
    _, nmul = sv.ldiv_(dx, lsq.DeviceVector(ctx, Jd.m, y), dd)
    x, info = dx.get(), sv.info()
    damp_after = dd.get() if dd is not None else None
    sv.free()
    Jd.free()
    assert nmul == 1 and info["blockdiag_path"] == "batched-qr"
    return x, info, damp_after


@pytest.mark.parametrize("nb", rc.BQ_NBS)
@pytest.mark.parametrize("mb", rc.BQ_MBS)
def test_blockqr_undamped(ctx, mb, nb):
    """Nine blocks (rc.bq_batch), every one judged as its own piece and every entry of block_ranks checked: one wavefront per
    block (nb <= 16) and one workgroup per block, mb < nb (3), one chunk of rows and several."""
    blocks = rc.bq_batch(mb, nb)
    x, info, _ = bq_solve(ctx, blocks)
    what = "blockqr undamped %dx%d" % (mb, nb)
    pieces, want = [], []
    for b, blk in enumerate(blocks):
        xb = x[b * nb:(b + 1) * nb]
        x_orc, rk, _ = rc.oracle_solve(blk.A, blk.y)
        assert rk == blk.rank, (what, b, blk.kind, rk)
        want.append(rk)
        if blk.kind == "zero":
            assert np.all(xb == 0.0), (what, b)
        elif blk.kind == "T":
            blk.tref.judge("rankdef %s block %d (T)" % (what, b), xb)
        else:
            pieces.append(("block %d (%s)" % (b, blk.kind), rc.rel_err(xb, blk.x_hp), rc.rel_err(x_orc, blk.x_hp), nb))
    print("PATH %s | %s ranks %s (oracle %s)" % (what, info["blockdiag_path"], list(info["block_ranks"]), want))
    assert list(info["block_ranks"]) == want and info["qr_rank"] == sum(want), (what, info["block_ranks"], want)
    ac.judge("rankdef " + what, pieces)


@pytest.mark.parametrize("nb", rc.BQ_NBS)
@pytest.mark.parametrize("mb", rc.BQ_MBS)
def test_blockqr_damped(ctx, mb, nb):
    """The same batches through the for_lm solver with damp = 0.1 colsumabs2: exactly 0 on the zero column and on the whole
    all-zero block, so those stacked blocks are rank-deficient themselves (rank nb - 1 and 0); every other block has rank nb
    whatever the rank of J_b."""
    blocks, refs = rc.bq_batch(mb, nb), rc.bq_damped_refs(mb, nb)
    damp = np.concatenate([zr.damp for zr in refs])
    x, info, damp_after = bq_solve(ctx, blocks, damp)
    what = "blockqr damped %dx%d" % (mb, nb)
    pieces, want = [], []
    for b, (blk, zr) in enumerate(zip(blocks, refs)):
        xb = x[b * nb:(b + 1) * nb]
        want.append(zr.rank_orc)
        assert zr.rank_orc == np.count_nonzero(np.any(blk.A != 0, axis=0)), (what, b, zr.rank_orc)
        zero = np.flatnonzero(zr.x_orc == 0.0)
        assert np.all(xb[zero] == 0.0), (what, b, xb[zero])
        if blk.kind != "zero":
            pieces.append(("block %d (%s)" % (b, blk.kind), zr.err(xb), zr.e_ref, nb))
    print("PATH %s | %s ranks %s (oracle %s)" % (what, info["blockdiag_path"], list(info["block_ranks"]), want))
    assert list(info["block_ranks"]) == want and info["qr_rank"] == sum(want), (what, info["block_ranks"], want)
    assert np.array_equal(damp_after, damp), what
    ac.judge("rankdef " + what, pieces)
