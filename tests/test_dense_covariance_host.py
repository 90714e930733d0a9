"""Dense parameter covariance, host tier (no device): the C entry point lsq_dense_covariance in header, loader and library, the
DenseCovariance container, the Julia shim's ccall in INTEGRATION.md, and the acceptance rule of
tests/test_j_gpu_dense_covariance.py checked on the CPU: on its eight shapes and every operand family both numpy.linalg.inv
and the fp64 stand-in of the device algorithm (ac.standin_inv: chunked Gram, Cholesky that multiplies by a reciprocal, explicit
inverse, X X') stay inside 16 max(e_ref, min(max(16, n), 64) 2^-53) -- the bound is within reach of a correct fp64
implementation -- while the stand-in with a float32-grade reciprocal square root does not: it is not vacuous either."""
import functools

import numpy as np
import pytest

import accuracy_common as ac
import hp_reference as hp
import julia_shim_lint as lint
import lsq_amd as lsq

SHAPES = [(40, 1), (50, 3), (90, 31), (200, 64), (300, 65), (500, 130), (700, 200), (1000, 321)]


def test_entry_point_declared_and_exported():
    assert "lsq_dense_covariance" in lsq.declared_symbols()
    L = lsq.lib()
    assert hasattr(L, "lsq_dense_covariance")
    ret, params = lint.header_prototypes()["lsq_dense_covariance"]
    assert ret == "int"
    assert params == lint.header_prototypes()["lsq_solver_covariance"][1]       # only the parameter types of its neighbour


def test_integration_ccall_present_and_typed():
    calls = [c for c in lint.ccalls() if c[0] == "lsq_dense_covariance"]
    assert len(calls) == 1
    name, ret, types, nvalues, line = calls[0]
    _, params = lint.header_prototypes()[name]
    assert "int" in lint.JULIA_CLASS[ret]
    assert nvalues == len(types) == len(params) == 6
    for t, p in zip(types, params):
        assert p in lint.JULIA_CLASS[t], (t, p)


def test_python_interface_is_exported():
    assert hasattr(lsq.AllocatedSolver, "dense_covariance")
    assert callable(lsq.dense_covariance)
    assert lsq.DenseCovariance.__name__ == "DenseCovariance"


def test_container_shapes_and_refusals():
    n = 4
    flat = np.arange(n * n, dtype=np.float64)
    c = lsq.DenseCovariance(n, flat, np.arange(n, dtype=np.float64))
    assert c.n == n and c.cov.shape == (n, n) and c.stderr.shape == (n,)
    assert c.cov[1, 2] == flat[2 * n + 1]                    # column-major, as the library writes it
    c2 = lsq.DenseCovariance(n, flat.reshape(n, n))
    assert c2.stderr is None and np.array_equal(c2.cov, flat.reshape(n, n))
    for bad in (np.zeros(15), np.zeros(17), np.zeros((2, 8)), np.zeros((n, n, 1))):
        with pytest.raises(lsq.DimensionMismatch):
            lsq.DenseCovariance(n, bad)
    for bad in (np.zeros(3), np.zeros(5), np.zeros((n, 1))):
        with pytest.raises(lsq.DimensionMismatch):
            lsq.DenseCovariance(n, flat, stderr=bad)


@functools.lru_cache(maxsize=None)
def shape_pieces(m, n):
    """Per family: (label, e_standin, e_degraded, e_numpy, bound floor k) for the covariance and the stderr piece."""
    out = []
    for family in ac.FAMILIES:
        if family == "graded" and n == 1:
            continue                                          # (ac.grading divides by k - 1)
        op = ac.dense_operand(family, m, n, ac.dense_seed(m, n))
        A, f = op.J, op.y
        H = hp.inv_gram(A) * ac.s2_of(f, m - n)
        s2 = float(f @ f) / (m - n)
        R = s2 * np.linalg.inv(A.T @ A)
        out.append((family, s2 * ac.standin_inv(A), s2 * ac.standin_inv(A, degraded=True), R, H))
    return out


@pytest.mark.parametrize("m,n", SHAPES)
def test_rule_is_within_reach_and_not_vacuous(m, n):
    degraded_rejected = 0
    for family, Cs, Cd, R, H in shape_pieces(m, n):
        label = "host stand-in %s %dx%d" % (family, m, n)
        ac.judge(label, ac.cov_pieces("standin", Cs, np.sqrt(np.diag(Cs)), R, H, n))
        ac.judge(label + " numpy", ac.cov_pieces("numpy", R, np.sqrt(np.diag(R)), R, H, n))
        e_ref = ac.cov_err(R, H)
        if not ac.accepted(ac.cov_err(Cd, H), e_ref, n):
            degraded_rejected += 1
    # a reciprocal square root good to 2^-24 only is 2^29 roundings off: the rule turns it away wherever LAPACK itself is
    # accurate (every family but ill, whose e_ref is cond(G) u)
    assert degraded_rejected >= len(shape_pieces(m, n)) - 1, (m, n, degraded_rejected)
