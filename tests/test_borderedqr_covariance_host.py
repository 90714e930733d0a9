"""No device: certifies the cases of tests/test_w_gpu_borderedqr_covariance.py.  The numpy fp64 twin of
lsq_bordered_qr_covariance (borderedqr_cov_common.twin: the device's steps in fp64) passes the accuracy tier's rule on every
committed case, with and without the variance and as a column-scaled handle; the fp64 normal-equations route is beyond the
bound on every ill6 case (so the cases tell a Gram-forming covariance from this one); two planted mistakes in the twin are
caught by the rule; and the failure cases fail where the device test expects them to.

Distances to the bound measured with this file (worst e_dev / bound over the cases of a family): see the printed ACC lines
of test_twin_passes_the_rule."""
import numpy as np
import pytest

import accuracy_common as ac
import borderedqr_common as bqc
import borderedqr_cov_common as bc


@pytest.mark.parametrize("case", bc.CASES, ids=bc.case_id)
def test_twin_passes_the_rule(case):
    family, shape = case
    op, ref = bc.operand(family, shape), bc.ref(family, shape)
    parts, fail, rank = bc.twin(op.J)
    assert fail == 0 and rank == shape[3]
    for with_f in (False, True):
        p = parts.scaled(ref.s2) if with_f else parts
        pieces = ref.pieces(p, with_f)
        assert len(pieces) == 3 * shape[0] + 2
        print("   fraction of the bound: %.3f" % bc.beyond(pieces))
        ac.judge("twin %s %s%s" % (family, shape, " with f" if with_f else ""), pieces)
    if family == "graded":
        parts, fail, _ = bc.twin(op.V, colscale=op.s)
        assert fail == 0
        ac.judge("twin %s %s colscale" % (family, shape), bc.ref(family, shape, True).pieces(parts, False))


@pytest.mark.parametrize("shape", bqc.ILL6_SHAPES)
def test_normal_equations_are_beyond_the_bound_on_ill6(shape):
    ref = bc.ref("ill6", shape)
    C = bc.normal_equations_route(ref.A)
    over = np.inf if C is None else bc.beyond(ref.pieces(bc.Parts.of_full(C, ref.B, ref.nb, ref.ng), False))
    print("normal equations on ill6 %s: %.3g x the bound" % (shape, over))
    assert over > 1.0


@pytest.mark.parametrize("plant", ["cross-sign", "no-border-term"])
@pytest.mark.parametrize("case", [("plain", (3, 40, 5, 31)), ("ill6", (5, 96, 5, 3))], ids=bc.case_id)
def test_the_rule_catches_a_planted_mistake(case, plant):
    family, shape = case
    op, ref = bc.operand(family, shape), bc.ref(family, shape)
    parts, _, _ = bc.twin(op.J, plant=plant)
    pieces = ref.pieces(parts, False)
    word = "cross" if plant == "cross-sign" else "block"
    bad = [p for p in pieces if not ac.accepted(p[1], p[2], p[3])]
    assert bad and all(p[0].startswith(word) for p in bad), (plant, [p[0] for p in bad])
    with pytest.raises(AssertionError):
        ac.judge("planted %s" % plant, pieces)


@pytest.mark.parametrize("name", bqc.RANK_CASES)
def test_twin_names_the_failing_local_column(name):
    J, _, _, expect = bqc.rank_case(name)
    parts, fail, _ = bc.twin(J)
    assert parts is None and fail == expect > 0


def test_duplicated_border_column_has_rank_ng_minus_one():
    J = bc.duplicated_border_case()
    with np.errstate(all="ignore"):
        _, fail, rank = bc.twin(J)
    assert fail == 0 and rank == J.ng - 1


def test_parts_of_full_and_distances():
    ref = bc.ref("plain", (3, 40, 5, 31))
    full = bc.Parts.of_full(ref.R, ref.B, ref.nb, ref.ng)
    assert full.cross.shape == (15, 31) and len(full.blocks) == 3 and full.shared.shape == (31, 31)
    assert all(d == 0.0 for _, d in ref.distances(full, full, False))
    twin, _, _ = bc.twin(bc.operand("plain", (3, 40, 5, 31)).J)
    pieces = {n: (e, r, k) for n, e, r, k in ref.pieces(twin, False)}
    for name, d in ref.distances(twin, full, False):          # the triangle inequality the agreement tests rely on
        e, r, _ = pieces[name]
        assert d <= e + r + 1e-18, (name, d, e, r)
