"""No device: certifies the cases of tests/test_z_gpu_bordered_leverage.py.  The numpy fp64 twin of lsq_bordered_qr_leverage
(bordered_leverage_common.Factor: the device's steps in fp64) is inside the accuracy tier's rule with k = nb + ng on every
committed case -- J's own rows with and without the variance, the graded cases as column-scaled handles, new rows --; four
planted mistakes (the border term dropped, the sign of Z W_b flipped, the inner permutation left out, the column scale left
out) each put it outside; the fp64 normal equations are outside on ill6; the reference's leverages add up to n; and header,
loader, library, the Julia shim and the Python names carry the entry.

Every case of borderedqr_cov_common.CASES is within the twin's reach with the library's generator: none was replaced."""
import os

import numpy as np
import pytest

import accuracy_common as ac
import bordered_leverage_common as blc
import borderedqr_common as bqc
import julia_shim_lint as lint
import leverage_common as lc
import lsq_amd as lsq


# ------------------------------------------------------------------------------------------ interface
def test_entry_point_declared_exported_and_bound():
    name = "lsq_bordered_qr_leverage"
    assert name in lsq.declared_symbols() and hasattr(lsq.lib(), name)
    ret, params = lint.header_prototypes()[name]
    assert ret == "int" and len(lsq.lib()._signatures[name][1]) == 15 == len(params)
    calls = [c for c in lint.ccalls() if c[0] == name]
    assert len(calls) == 1
    _, jret, types, nvalues, _ = calls[0]
    assert "int" in lint.JULIA_CLASS[jret] and nvalues == len(types) == len(params)
    for t, p in zip(types, params):
        assert p in lint.JULIA_CLASS[t], (t, p)


def test_python_interface_is_exported():
    assert hasattr(lsq.AllocatedSolver, "bordered_qr_leverage") and callable(lsq.bordered_qr_leverage)
    lev = lsq.Leverage(np.arange(6.0), se=np.ones(6), s2=2.5, rank=4, nblocks=2, mb=3)      # one variance, no per-block info
    blk = lev.block(1)
    assert np.array_equal(blk.q, [3.0, 4.0, 5.0]) and blk.s2 == 2.5 and blk.info is None and blk.rank == 4 and blk.cook is None
    assert lsq.Leverage(np.arange(6.0), nblocks=2, mb=3).block(0).s2 is None
    with pytest.raises(IndexError):
        lev.block(2)


def test_kernel_is_built_from_the_makefile():
    csrc = os.path.join(lsq._lib.ROOT, "leastsquaresoptim.jl_amd", "csrc")
    assert "lsq_lev_bordered.hip" in open(os.path.join(csrc, "Makefile")).read()
    src = open(os.path.join(csrc, "lsq_lev_bordered.hip")).read()
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64" in src and "k_bl_local" in src and "k_lev_tall" in src


# ------------------------------------------------------------------------------------------ the rule on every case
@pytest.mark.parametrize("case", blc.CASES, ids=blc.case_id)
def test_twin_is_within_the_rule(case):
    family, shape = case
    B, mb, nb, ng = shape
    op, r = blc.operand(family, shape), blc.ref(family, shape)
    # the reference itself: the trace of the hat matrix, every leverage inside (0, 1]
    assert abs(float(np.sum(r.q_hp)) - r.n) <= 1e-12 * r.n
    assert np.all(r.q_hp > 0) and np.all(r.q_hp <= 1 + 1e-15)
    fac = blc.Factor(op.J)
    q = fac.own()
    label = "host bordered leverage %s %s" % (family, shape)
    with_f = r.m > r.n
    pcs = blc.pieces("twin", q, r, with_f, np.sqrt(r.s2) * np.sqrt(q) if with_f else None)
    print("   fraction of the bound: %.3f" % blc.beyond(pcs))
    blc.judge(label, pcs)
    if family == "graded":
        rs = blc.ref(family, shape, True)
        blc.judge(label + " colscale", blc.pieces("twin", blc.twin(op.V, colscale=op.s), rs))
    # new rows of the first and the last block
    for b in sorted({0, B - 1}):
        Al, Ag = blc.new_rows(op.J, b, 7, 50 + b)
        rr = blc.Ref(op, A=blc.full_rows(op.J, b, Al, Ag))
        blc.judge(label + " new rows of block %d" % b, blc.pieces("rows", fac.q(b, Al, Ag), rr))


# ------------------------------------------------------------------------------------------ planted mistakes
@pytest.mark.parametrize("plant", [p for p in blc.PLANTS if p != "no-colscale"])
@pytest.mark.parametrize("case", [("plain", (3, 40, 5, 31)), ("plain", (3, 100, 17, 65)), ("ill6", (5, 96, 5, 3))], ids=blc.case_id)
def test_the_rule_catches_a_planted_mistake(case, plant):
    family, shape = case
    op, r = blc.operand(family, shape), blc.ref(family, shape)
    good, bad = blc.pieces("twin", blc.twin(op.J), r), blc.pieces("planted", blc.twin(op.J, plant=plant), r)
    print("PLANTED %s %s %s: %.3g x the bound" % (plant, family, shape, blc.beyond(bad)))
    assert blc.beyond(good) <= 1.0 < blc.beyond(bad)


@pytest.mark.parametrize("shape", [(3, 40, 5, 31), (3, 100, 17, 65)])
def test_the_rule_catches_a_missing_column_scale(shape):
    op, rs = blc.operand("graded", shape), blc.ref("graded", shape, True)
    assert blc.beyond(blc.pieces("twin", blc.twin(op.V, colscale=op.s), rs)) <= 1.0
    assert blc.beyond(blc.pieces("planted", blc.twin(op.V, colscale=op.s, plant="no-colscale"), rs)) > 1.0


@pytest.mark.parametrize("shape", bqc.ILL6_SHAPES)
def test_normal_equations_are_beyond_the_bound_on_ill6(shape):
    r = blc.ref("ill6", shape)
    over = blc.beyond(blc.pieces("normal equations", blc.q_normal_equations(r.A), r))
    print("normal equations on ill6 %s: %.3g x the bound" % (shape, over))
    assert over > 1.0


def test_square_case_has_unit_leverages():
    r = blc.ref(*blc.SQUARE)
    assert r.m == r.n == 2 and r.s2 is None
    assert np.all(np.abs(np.asarray(r.q_hp, dtype=np.float64) - 1.0) <= 1e-15)
    assert np.all(np.abs(blc.twin(blc.operand(*blc.SQUARE).J) - 1.0) <= 1e-12)
