"""optimize_batched_ / lsq_optimize_batched, the part that needs no device: the ctypes mirror of lsq_batched_result against
the header (the technique of test_host.py::test_julia_shim_matches_the_header), the exported symbol, BatchedResult.block(b)
on a hand-made result, and every refusal that happens before a device call."""
import ctypes as C

import numpy as np
import pytest

import lsq_amd as lsq


def test_ctypes_mirror_matches_the_header():
    import julia_shim_lint as JL
    cf = JL.header_struct("lsq_batched_result")
    mirror = lsq._lib.BatchedResult._fields_
    assert [f for f, _ in mirror] == [f for f, _ in cf]
    cls = {C.c_int: "int", C.c_double: "double", lsq._lib.c_dp: "ptr:double", lsq._lib.c_ip: "ptr:int"}
    for (f, t), (_, ct) in zip(mirror, cf):
        assert cls[t] == ct, (f, t, ct)
    # lsq_options / lsq_result keep their layout (the new entry point takes the existing options struct)
    assert [f for f, _ in lsq._lib.Options._fields_] == [f for f, _ in JL.header_struct("lsq_options")]
    assert [f for f, _ in lsq._lib.Result._fields_] == [f for f, _ in JL.header_struct("lsq_result")]


def test_entry_point_is_declared_and_exported():
    assert "lsq_optimize_batched" in lsq.declared_symbols()
    L = lsq.lib()
    assert hasattr(L, "lsq_optimize_batched") and "lsq_optimize_batched" in L._signatures
    import julia_shim_lint as JL
    ret, params = JL.header_prototypes()["lsq_optimize_batched"]
    assert ret == "int" and len(params) == 11 and params[-2] == "ptr:lsq_options"
    assert any(c[0] == "lsq_optimize_batched" for c in JL.ccalls())          # INTEGRATION.md binds it


def test_block_slicing_on_a_hand_made_result():
    B, mb, nb, cap = 3, 4, 2, 5
    r = lsq.BatchedResult(B, mb, nb, "Dogleg", 1e-7, 1e-6, 1e-5)
    r.ssr[:] = [1.0, 2.0, 3.0]
    r.ssr0[:] = [10.0, 20.0, 30.0]
    r.iterations[:] = [2, 5, 0]
    r.converged[:] = [1, 0, 0]
    r.f_converged[:] = [1, 0, 0]
    r.f_calls[:] = [3, 6, 1]
    r.g_calls[:] = [2, 3, 0]
    r.mul_calls[:] = [7, 14, 0]
    r.status[:] = [0, 0, lsq._lib.ENONFINITE]
    r.info[:] = [-1, -1, 1]
    r.minimizer = np.arange(B * nb, dtype=float)
    acc = np.array([[1, 0, 0], [1, 1, 0], [0, 0, 0], [0, 1, 0], [0, 1, 0]], dtype=np.int32)
    r.trace = dict(ssr=np.arange(cap * B, dtype=float).reshape(cap, B), gnorm=np.ones((cap, B)), delta=np.ones((cap, B)),
                   rho=np.ones((cap, B)), accept=acc, x=np.arange(cap * B * nb, dtype=float).reshape(cap, B * nb))
    b0, b1, b2 = r.block(0), r.block(1), r.block(2)
    assert (b0.iterations, b0.converged, b0.f_converged, b0.x_converged, b0.g_converged) == (2, True, True, False, False)
    assert (b0.f_calls, b0.g_calls, b0.mul_calls, b0.status, b0.info) == (3, 2, 7, 0, -1)
    assert (b0.x_tol, b0.f_tol, b0.g_tol, b0.optimizer) == (1e-7, 1e-6, 1e-5, "Dogleg")
    assert np.array_equal(b1.minimizer, [2.0, 3.0]) and b1.ssr == 2.0 and b1.ssr0 == 20.0
    assert b0.trace["ssr"].tolist() == [0.0, 3.0] and b0.trace["x"].shape == (2, nb)
    assert np.array_equal(b1.trace["x"][4], r.trace["x"][4, 2:4]) and len(b1.trace["ssr"]) == 5
    assert b1.trace["accept"].tolist() == [0, 1, 0, 1, 1]
    assert b1.trace["inner"].tolist() == [1, 0, 1, 0, 1]        # Dogleg solves again only after an accepted step
    assert (b2.iterations, b2.status, b2.info) == (0, lsq._lib.ENONFINITE, 1) and len(b2.trace["ssr"]) == 0
    r.optimizer = "LevenbergMarquardt"
    assert r.block(1).trace["inner"].tolist() == [1, 1, 1, 1, 1]
    with pytest.raises(IndexError):
        r.block(3)


def test_refusals_before_any_device_call():
    f = lambda out, x: None
    g = lambda J, x: None
    J = lsq.BlockDiagonal(4, 16, 8)
    nls = lambda JJ, n=32: lsq.LeastSquaresProblem(x=np.zeros(n), f_=f, g_=g, J=JJ)
    for bad in (np.zeros((64, 32)), J.tocsc()):
        with pytest.raises(lsq.ArgumentError) as e:
            lsq.optimize_batched_(nls(bad))
        assert e.value.status == lsq._lib.EARG and "BlockDiagonal" in str(e.value)
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.optimize_batched_(nls(J), lsq.Dogleg(lsq.QR()))
    assert str(e.value) == "solver QR() is not available for sparse Jacobians. Choose between Cholesky() and LSMR()"
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.optimize_batched_(nls(J), lsq.LevenbergMarquardt(lsq.LSMR()))
    assert e.value.status == lsq._lib.EARG and "LSMR() is not available per block" in str(e.value)
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.optimize_batched_(nls(lsq.BlockDiagonal(2, 70, 65), 130))
    assert "64" in str(e.value) and "65" in str(e.value)
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.optimize_batched_(nls(J), lower=np.zeros(5))
    assert "Bounds must either be empty" in str(e.value)
    assert lsq.optimize_batched_.__defaults__[0] is None      # default optimizer resolved per call: LevenbergMarquardt(Cholesky())
    opt, solver = lsq.api._batched_arguments(J, None, 32, (), ())
    assert isinstance(opt, lsq.LevenbergMarquardt) and isinstance(solver, lsq.Cholesky)
    opt, solver = lsq.api._batched_arguments(J, lsq.Dogleg(), 32, (), ())
    assert isinstance(opt, lsq.Dogleg) and isinstance(solver, lsq.Cholesky)
