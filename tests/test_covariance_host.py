"""Parameter covariance, host tier (no device): the C entry point lsq_solver_covariance in header, loader and library, the
Covariance container's views and shapes, and the Julia shim's ccall in INTEGRATION.md."""
import numpy as np
import pytest

import julia_shim_lint as lint
import lsq_amd as lsq


def test_entry_point_declared_and_exported():
    assert "lsq_solver_covariance" in lsq.declared_symbols()
    L = lsq.lib()
    assert hasattr(L, "lsq_solver_covariance")
    res, args = L._signatures["lsq_solver_covariance"]
    assert len(args) == 6
    ret, params = lint.header_prototypes()["lsq_solver_covariance"]
    assert ret == "int"
    assert params == ["ptr:void", "ptr:void", "ptr:double", "ptr:double", "ptr:double", "ptr:int"]


def test_integration_ccall_present_and_typed():
    calls = [c for c in lint.ccalls() if c[0] == "lsq_solver_covariance"]
    assert len(calls) == 1
    name, ret, types, nvalues, line = calls[0]
    _, params = lint.header_prototypes()[name]
    assert "int" in lint.JULIA_CLASS[ret]
    assert nvalues == len(types) == len(params) == 6
    for t, p in zip(types, params):
        assert p in lint.JULIA_CLASS[t], (t, p)


def test_python_interface_is_exported():
    assert hasattr(lsq.AllocatedSolver, "covariance")
    assert callable(lsq.covariance)
    assert lsq.Covariance.__name__ == "Covariance"


def test_container_blockdiag_views_and_shapes():
    B, nb = 3, 4
    cov = np.arange(B * nb * nb, dtype=np.float64)
    se = np.arange(B * nb, dtype=np.float64)
    c = lsq.Covariance(B, nb, 0, cov, se, info=[0, 2, 0])
    assert c.shared is None
    assert c.stderr.shape == (B * nb,) and np.array_equal(c.stderr, se)
    assert c.info.dtype == np.int32 and list(c.info) == [0, 2, 0]
    for b in range(B):
        blk = c.block(b)
        assert blk.shape == (nb, nb)
        assert np.array_equal(blk, cov[b * nb * nb:(b + 1) * nb * nb].reshape(nb, nb))      # row-major, block after block
        assert np.shares_memory(blk, c.cov)                                                   # a view
    c.block(1)[2, 3] = -7.0
    assert c.cov[nb * nb + 2 * nb + 3] == -7.0
    for bad in (-1, B):
        with pytest.raises(IndexError):
            c.block(bad)


def test_container_bordered_views_and_shapes():
    B, nb, ng = 2, 3, 2
    cov = np.arange(B * nb * nb + ng * ng, dtype=np.float64)
    c = lsq.Covariance(B, nb, ng, cov)
    assert c.stderr is None and c.info is None
    assert c.block(1).shape == (nb, nb) and c.block(1)[0, 0] == nb * nb
    assert c.shared.shape == (ng, ng)
    assert np.array_equal(c.shared, cov[B * nb * nb:].reshape(ng, ng))
    assert np.shares_memory(c.shared, c.cov)


def test_container_refuses_wrong_lengths():
    with pytest.raises(lsq.DimensionMismatch):
        lsq.Covariance(2, 3, 0, np.zeros(17))
    with pytest.raises(lsq.DimensionMismatch):
        lsq.Covariance(2, 3, 1, np.zeros(19), stderr=np.zeros(6))
