"""Dense covariance from the QR() factor, host tier (no device): the C entry point lsq_dense_qr_covariance in header, loader and
library, the Julia shim's ccall, the Python names, and the acceptance rule of tests/test_n_gpu_dense_qr_covariance.py checked
on the CPU (tests/qr_cov_common.py): on its seven shapes and every operand family two fp64 QR routes -- e_ref's own
(numpy.linalg.qr, a triangular solve, X X') and the device's algebra (pivoted LAPACK QR, block-recursive inverse, X X',
un-permute) -- stay inside 16 max(e_ref, min(max(16, n), 64) 2^-53), so the bound is within reach of a correct fp64
implementation; numpy.linalg.inv(A.T @ A), the normal-equation route the library offered before, is turned away on every
ill-conditioned operand, so it is not vacuous either.  Also: on the 3-decade operands the longdouble reference from the
Householder R agrees with hp.inv_gram (longdouble Cholesky of J'J, which still has digits there) to 1e-12."""
import numpy as np
import pytest

import accuracy_common as ac
import hp_reference as hp
import julia_shim_lint as lint
import lsq_amd as lsq
import qr_cov_common as qc


def test_entry_point_declared_and_exported():
    assert "lsq_dense_qr_covariance" in lsq.declared_symbols()
    L = lsq.lib()
    assert hasattr(L, "lsq_dense_qr_covariance")
    protos = lint.header_prototypes()
    assert protos["lsq_dense_qr_covariance"] == protos["lsq_dense_covariance"]
    assert protos["lsq_dense_qr_covariance"][0] == "int"


def test_integration_ccall_present_and_typed():
    calls = [c for c in lint.ccalls() if c[0] == "lsq_dense_qr_covariance"]
    assert len(calls) == 1
    name, ret, types, nvalues, line = calls[0]
    _, params = lint.header_prototypes()[name]
    assert "int" in lint.JULIA_CLASS[ret]
    assert nvalues == len(types) == len(params) == 6
    for t, p in zip(types, params):
        assert p in lint.JULIA_CLASS[t], (t, p)


def test_python_interface_is_exported():
    assert hasattr(lsq.AllocatedSolver, "dense_qr_covariance")
    assert callable(lsq.dense_qr_covariance)
    assert issubclass(lsq.RankDeficientException, lsq.LsqError)


@pytest.mark.parametrize("m,n", qc.SHAPES)
def test_rule_is_within_reach_and_not_vacuous(m, n):
    for family in qc.FAMILIES:
        if (m, n, family) not in qc.CASES:
            continue
        r = qc.ref(family, m, n)
        for with_f in (False, True):
            s64 = r.scales(with_f)[1]
            label = "host %s %dx%d %s" % (family, m, n, "f" if with_f else "unscaled")
            Cq = s64 * r.R
            ac.judge(label + " qr", r.pieces("qr", Cq, np.sqrt(np.diag(Cq)), with_f))
            Cp = s64 * qc.fp64_pivoted_route(r.A)
            ac.judge(label + " pivoted qr", r.pieces("pivoted", Cp, np.sqrt(np.diag(Cp)), with_f))
        # the normal equations: cond(A)^2 u against the QR routes' cond(A) u.  (n = 1 has cond(A) = 1 in every family:
        # logspace(0, -d, 1) = [1], nothing to tell the routes apart by.)
        if family in qc.ILL_FAMILIES and n > 1:
            e_ref = ac.cov_err(r.R, r.H)
            try:
                e_ne = ac.cov_err(np.linalg.inv(r.A.T @ r.A), r.H)
            except np.linalg.LinAlgError:
                e_ne = np.inf
            print("NORMAL EQUATIONS %s %dx%d: e %.3e, e_ref %.3e, %.1f x the bound"
                  % (family, m, n, e_ne, e_ref, e_ne / ac.bound(e_ref, n)))
            assert not ac.accepted(e_ne, e_ref, n), (family, m, n, e_ne, e_ref)


@pytest.mark.parametrize("m,n", qc.SHAPES)
def test_reference_agrees_with_inv_gram_at_three_decades(m, n):
    r = qc.ref("ill", m, n)
    e = ac.cov_err(hp.inv_gram(r.A), r.H)
    print("longdouble references, ill %dx%d: %.3e apart" % (m, n, e))
    assert e <= 1e-12
