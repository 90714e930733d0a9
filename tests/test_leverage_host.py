"""Leverages and prediction variances, host tier (no device): the two C entry points in header, loader and library, the Julia
shim's ccalls, the Python names, and the acceptance rule of tests/test_y_gpu_leverage.py checked on the CPU
(tests/leverage_common.py): on every committed case the numpy twin of the device's algebra and the fp64 e_ref route stay
inside 16 max(e_ref, min(max(16, n), 64) 2^-53) of the longdouble reference, so the bound is within reach of a correct fp64
implementation; with a planted mistake -- the permutation left out or inverted, junk below the diagonal of X, K < Jt for
K <= Jt, the column scale left out -- the twin is beyond it, and so are the fp64 normal equations on ill6 and ill9, which is why
the entry point is built on the QR() factor; on the block handle one Cholesky of J_b'J_b is beyond it on `ill`, which is why
k_bd_lev is a CholeskyQR2."""
import numpy as np
import pytest

import accuracy_common as ac
import hp_reference as hp
import julia_shim_lint as lint
import leverage_common as lc
import lsq_amd as lsq
import qr_cov_common as qc


# ------------------------------------------------------------------------------------------ interface
def test_entry_points_declared_and_exported():
    declared = lsq.declared_symbols()
    L = lsq.lib()
    protos = lint.header_prototypes()
    for name, nargs in (("lsq_dense_qr_leverage", 12), ("lsq_solver_leverage", 9)):
        assert name in declared, name
        assert hasattr(L, name), name
        assert len(L._signatures[name][1]) == nargs == len(protos[name][1]), name
        assert protos[name][0] == "int"


def test_integration_ccalls_present_and_typed():
    for name in ("lsq_dense_qr_leverage", "lsq_solver_leverage"):
        calls = [c for c in lint.ccalls() if c[0] == name]
        assert len(calls) == 1, name
        _, ret, types, nvalues, line = calls[0]
        _, params = lint.header_prototypes()[name]
        assert "int" in lint.JULIA_CLASS[ret]
        assert nvalues == len(types) == len(params)
        for t, p in zip(types, params):
            assert p in lint.JULIA_CLASS[t], (name, t, p)


def test_python_interface_is_exported():
    assert hasattr(lsq.AllocatedSolver, "dense_qr_leverage") and hasattr(lsq.AllocatedSolver, "leverage")
    assert callable(lsq.dense_qr_leverage) and callable(lsq.leverage)
    lev = lsq.Leverage(np.arange(6.0), se=np.ones(6), s2=np.array([2.0, 3.0]), info=np.zeros(2, dtype=np.int32), nblocks=2, mb=3)
    assert lev.h is lev.q
    blk = lev.block(1)
    assert np.array_equal(blk.q, [3.0, 4.0, 5.0]) and blk.s2 == 3.0 and blk.cook is None and blk.se.shape == (3,)
    with pytest.raises(IndexError):
        lev.block(2)


def test_kernel_is_built_from_the_makefile():
    import os
    csrc = os.path.join(lsq._lib.ROOT, "leastsquaresoptim.jl_amd", "csrc")
    assert "lsq_leverage.hip" in open(os.path.join(csrc, "Makefile")).read()
    src = open(os.path.join(csrc, "lsq_leverage.hip")).read()
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64" in src and "lsq_dense_qr_cov_factor" in src


# ------------------------------------------------------------------------------------------ the rule on the dense cases
@pytest.mark.parametrize("m,n", qc.SHAPES)
def test_rule_is_within_reach_and_not_vacuous(m, n):
    for family in qc.FAMILIES:
        if (m, n, family) not in lc.CASES:
            continue
        r = lc.ref(family, m, n)
        # the reference itself: trace of the hat matrix, and every leverage inside (0, 1]
        assert abs(float(np.sum(r.q_hp)) - n) <= 1e-12 * n, (family, float(np.sum(r.q_hp)))
        assert np.all(r.q_hp > 0) and np.all(r.q_hp <= 1 + 1e-15)
        label = "host leverage %s %dx%d" % (family, m, n)
        q_twin = lc.twin_dense(r.J)
        for with_f in (False, True):
            ac.judge(label + (" f" if with_f else "") + " twin",
                     lc.pieces("twin", q_twin, r, with_f, np.sqrt(r.s2) * np.sqrt(q_twin)))
            ac.judge(label + (" f" if with_f else "") + " qr",
                     lc.pieces("qr", r.q_ref, r, with_f, np.sqrt(r.s2) * np.sqrt(r.q_ref)))
        if family in ("ill6", "ill9") and n > 1:     # (n = 1 has cond 1 in every family)
            e_ref = lc.lev_err(r.q_ref, r.q_hp)
            try:
                e_ne = lc.lev_err(lc.q_normal_equations(r.J), r.q_hp)
            except np.linalg.LinAlgError:
                e_ne = np.inf
            print("NORMAL EQUATIONS %s %dx%d: e %.3e, e_ref %.3e, %.1f x the bound"
                  % (family, m, n, e_ne, e_ref, e_ne / ac.bound(e_ref, n)))
            assert not ac.accepted(e_ne, e_ref, n), (family, m, n, e_ne, e_ref)


@pytest.mark.parametrize("m,n", [(300, 65), (500, 130)])
def test_new_rows(m, n):
    """Rows that were not measured: the same rule, p = 129 rows drawn like the operand's."""
    for family in ("plain", "shuffled-graded", "ill6"):
        J, f = qc.operand(family, m, n)
        rng = np.random.default_rng(m + n)
        A = np.asfortranarray(J[rng.integers(0, m, 129)] * (1.0 + 0.5 * rng.standard_normal((129, 1))))
        r = lc.Ref(J, f, A=A)
        ac.judge("host leverage new rows %s %dx%d" % (family, m, n), lc.pieces("twin", lc.twin_dense(J, A), r))


# ------------------------------------------------------------------------------------------ planted mistakes
@pytest.mark.parametrize("mistake", [k for k in lc.MISTAKES if k != "no-colscale"])
@pytest.mark.parametrize("m,n", [(300, 65), (500, 130)])
def test_planted_mistakes_are_beyond_the_bound(m, n, mistake):
    r = lc.ref("shuffled-graded", m, n)
    q = lc.twin_dense(r.J, mistake=mistake)
    e, e_ref = lc.lev_err(q, r.q_hp), lc.lev_err(r.q_ref, r.q_hp)
    print("PLANTED %s %dx%d: e %.3e against the bound %.3e" % (mistake, m, n, e, ac.bound(e_ref, n)))
    assert not ac.accepted(e, e_ref, n)
    assert ac.accepted(lc.lev_err(lc.twin_dense(r.J), r.q_hp), e_ref, n)


def test_planted_missing_column_scale():
    m, n = 300, 65
    V, f = qc.operand("plain", m, n)
    s = ac.grading(n)
    r = lc.Ref(np.asfortranarray(V * s), f, J_eff=hp.ld(V) * hp.ld(s))
    good = lc.twin_dense(r.J, A=V, scale=s)
    bad = lc.twin_dense(r.J, A=V, scale=s, mistake="no-colscale")
    e_ref = lc.lev_err(r.q_ref, r.q_hp)
    assert ac.accepted(lc.lev_err(good, r.q_hp), e_ref, n)
    assert not ac.accepted(lc.lev_err(bad, r.q_hp), e_ref, n)


# ------------------------------------------------------------------------------------------ block-diagonal cases
@pytest.mark.parametrize("family", ac.FAMILIES)
@pytest.mark.parametrize("nb", ac.BD_NBS)
def test_block_rule_is_within_reach(nb, family):
    """The block twin (CholeskyQR2 on the streamed Gram, as k_bd_lev has it) against the same rule, e_ref from the fp64 QR
    route.  On `ill` (cond(J_b) = 1e3) ONE Cholesky of J_b'J_b (cond 1e6) is 10 to 70 x beyond the bound at every nb, which is
    why the kernel makes the second pass; that is asserted too, so the case keeps telling the two apart."""
    B, mb = ac.BD_B, ac.BD_MB
    op = ac.bd_operand(family, B, mb, nb, ac.bd_seed(nb))
    out = []
    for b in range(B):
        r = lc.block_ref(op, b)
        assert abs(float(np.sum(r.q_hp)) - nb) <= 1e-12 * nb and np.all(r.q_hp > 0) and np.all(r.q_hp <= 1 + 1e-15)
        h = lc.twin_block(r.J)
        out += lc.pieces("block %d" % b, h, r, True, np.sqrt(r.s2) * np.sqrt(h))
    ac.judge("host block leverage %s nb=%d" % (family, nb), out)
    if family == "ill":
        r = lc.block_ref(op, 0)
        assert not ac.accepted(lc.lev_err(lc.twin_block(r.J, second_pass=False), r.q_hp), lc.lev_err(r.q_ref, r.q_hp), nb)


# ------------------------------------------------------------------------------------------ the elementwise twin
def test_diag_twin_agrees_with_longdouble():
    rng = np.random.default_rng(7)
    m, n = 1000, 9
    q = rng.random(m) * 0.9 + 1e-3
    f = rng.standard_normal(m)
    s2 = float(f @ f) / (m - n)
    got = lc.diag_twin(q, f, s2, n)
    want = lc.diag_hp(q, f, s2, n)
    # se: 3 roundings; t: 5; cook: t twice, 3 more (1 - q is exact to half an ulp of d, and d >= 0.1 here)
    for g, w, ulps in zip(got, want, (4, 8, 24)):
        assert np.all(np.abs(hp.ld(g) - w) <= ulps * ac.UNIT * np.abs(w))
    # per-row variances (the block handle) and the IEEE results where h rounds to 1 or beyond: nothing is clamped
    se, t, cook = lc.diag_twin(np.array([1.0, 1.0 + 2.0 ** -52, 0.5]), np.array([0.0, 1.0, 1.0]), np.array([2.0, 2.0, 8.0]), 3)
    assert np.isnan(t[0]) and np.isnan(cook[0])                  # 0 / 0
    assert np.isnan(t[1]) and np.isnan(cook[1])                  # sqrt of a negative number
    assert se[2] == np.sqrt(8.0) * np.sqrt(0.5) and t[2] == 1.0 / (np.sqrt(8.0) * np.sqrt(0.5))
    se, t, cook = lc.diag_twin(np.array([1.0]), np.array([1.0]), 2.0, 3)
    assert np.isposinf(t[0]) and np.isposinf(cook[0])            # f / 0, then inf * 1 / 0
