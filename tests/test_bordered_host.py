"""Bordered block-diagonal Jacobians, host tier (no device): the BorderedBlockDiagonal container, the solver / optimizer
defaults and refusals on it, and the two C entry points (lsq_blockdiag_bordered_create, lsq_mat_bordered_info) in header,
loader and library."""
import numpy as np
import pytest

import lsq_amd as lsq


def _random(B, mb, nb, ng, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((mb, nb)) for _ in range(B)], rng.standard_normal((B * mb, ng))


@pytest.mark.parametrize("B,mb,nb,ng", [(1, 1, 1, 1), (3, 5, 2, 2), (4, 2, 6, 1), (7, 9, 3, 5)])
def test_layout_is_the_csc_layout(B, mb, nb, ng):
    blocks, border = _random(B, mb, nb, ng, 10 * B + nb)
    J = lsq.BorderedBlockDiagonal.from_blocks(blocks, border)
    assert (J.nblocks, J.mb, J.nb, J.ng) == (B, mb, nb, ng)
    assert J.shape == (B * mb, B * nb + ng) and J.nnz == B * mb * (nb + ng) == J.data.size
    # B column-major blocks back to back, then ng columns of m values
    assert np.array_equal(J.data, np.concatenate([b.reshape(-1, order="F") for b in blocks] + [border.reshape(-1, order="F")]))
    S = J.tocsc()
    assert S.shape == J.shape and S.nnz == J.nnz and S.has_sorted_indices
    assert np.array_equal(S.data, J.data)              # the nzval order of the equivalent sparse matrix
    assert S.data is not J.data
    dense = np.zeros(J.shape)
    for b, blk in enumerate(blocks):
        dense[b * mb:(b + 1) * mb, b * nb:(b + 1) * nb] = blk
    dense[:, B * nb:] = border
    assert np.array_equal(S.toarray(), dense) and np.array_equal(J.toarray(), dense)


def test_views_alias_data_and_round_trip():
    B, mb, nb, ng = 5, 4, 3, 2
    blocks, border = _random(B, mb, nb, ng, 1)
    J = lsq.BorderedBlockDiagonal.from_blocks(blocks, border)
    for b, blk in enumerate(blocks):
        assert np.array_equal(J.block(b), blk)
        assert np.array_equal(J.border_block(b), border[b * mb:(b + 1) * mb])
    assert np.array_equal(J.border, border)
    v, c, cb = J.block(2), J.border, J.border_block(3)
    assert np.shares_memory(v, J.data) and np.shares_memory(c, J.data) and np.shares_memory(cb, J.data)
    assert v.shape == (mb, nb) and c.shape == (B * mb, ng) and cb.shape == (mb, ng)
    v[1, 2] = 77.0
    assert J.data[2 * 12 + 2 * 4 + 1] == 77.0
    c[7, 1] = -3.0                                     # row 7 of border column 1
    assert J.data[B * mb * nb + 1 * B * mb + 7] == -3.0
    cb[0, 0] = 9.0                                     # row 3*mb of border column 0
    assert J.data[B * mb * nb + 3 * mb] == 9.0 and J.border[3 * mb, 0] == 9.0
    # g! may rebind .data: the views follow the binding
    J.data = np.arange(J.nnz, dtype=np.float64)
    assert J.block(1)[0, 0] == 12.0 and J.border[0, 0] == B * mb * nb and J.border_block(4)[3, 1] == J.nnz - 1
    K = lsq.BorderedBlockDiagonal(B, mb, nb, ng, data=J.data)
    assert np.array_equal(K.toarray(), J.toarray())
    Z = lsq.BorderedBlockDiagonal(2, 3, 2, 1)
    assert Z.data.shape == (18,) and not Z.data.any()


def test_dimension_errors():
    for args in ((0, 3, 2, 1), (2, 0, 2, 1), (2, 3, -1, 1), (2, 3, 2, 0)):
        with pytest.raises(lsq.DimensionMismatch):
            lsq.BorderedBlockDiagonal(*args)
    with pytest.raises(lsq.DimensionMismatch):
        lsq.BorderedBlockDiagonal(2, 3, 2, 1, data=np.zeros(17))
    with pytest.raises(lsq.DimensionMismatch):
        lsq.BorderedBlockDiagonal.from_blocks([np.zeros((3, 2)), np.zeros((2, 3))], np.zeros((6, 1)))
    with pytest.raises(lsq.DimensionMismatch):
        lsq.BorderedBlockDiagonal.from_blocks([], np.zeros((6, 1)))
    with pytest.raises(lsq.DimensionMismatch):
        lsq.BorderedBlockDiagonal.from_blocks([np.zeros((3, 2))] * 2, np.zeros((5, 1)))
    with pytest.raises(IndexError):
        lsq.BorderedBlockDiagonal(2, 3, 2, 1).block(2)
    with pytest.raises(IndexError):
        lsq.BorderedBlockDiagonal(2, 3, 2, 1).border_block(-1)
    J = lsq.BorderedBlockDiagonal(2, 3, 2, 1)
    f_ = lambda out, x: None
    with pytest.raises(lsq.DimensionMismatch):
        lsq.LeastSquaresProblem(x=np.zeros(4), y=np.zeros(6), f_=f_, g_=lambda J, x: None, J=J)
    nls = lsq.LeastSquaresProblem(x=np.zeros(5), f_=f_, g_=lambda J, x: None, J=J)
    assert nls.J is J and len(nls.y) == 6


def test_default_solver_and_optimizer():
    J = lsq.BorderedBlockDiagonal(3, 4, 2, 2)
    s = lsq.default_solver(None, J)
    assert isinstance(s, lsq.LSMR)
    assert isinstance(lsq.default_optimizer(None, s, J), lsq.LevenbergMarquardt)
    assert isinstance(lsq.default_optimizer(lsq.Dogleg(), s, J), lsq.Dogleg)          # Dogleg(LSMR()) is the CSC path
    c = lsq.default_solver(lsq.Cholesky(), J)
    assert isinstance(c, lsq.Cholesky)
    o = lsq.default_optimizer(None, c, J)                                              # not Dogleg: it does not exist here
    assert isinstance(o, lsq.LevenbergMarquardt) and o.solver is c
    assert isinstance(lsq.default_optimizer(lsq.LevenbergMarquardt(), c, J), lsq.LevenbergMarquardt)
    # other Jacobians keep the reference's defaults
    assert isinstance(lsq.default_optimizer(None, lsq.Cholesky()), lsq.Dogleg)
    assert isinstance(lsq.default_optimizer(None, lsq.Cholesky(), lsq.BlockDiagonal(3, 4, 2)), lsq.Dogleg)


def _problem(J):
    return lsq.LeastSquaresProblem(x=np.zeros(J.shape[1]), f_=lambda o, x: None, g_=lambda J, x: None, J=J)


def test_refusals_need_no_device():
    J = lsq.BorderedBlockDiagonal(3, 4, 2, 2)
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.default_solver(lsq.QR(), J)
    assert e.value.status == lsq._lib.EARG
    assert "BorderedBlockDiagonal" in str(e.value) and "Cholesky()" in str(e.value) and "LSMR()" in str(e.value)
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.default_solver(lsq.BlockQR(), J)
    assert "BlockQR()" in str(e.value) and "BorderedBlockDiagonal" in str(e.value)
    K = lsq.BorderedBlockDiagonal(2, 70, 60, 5)
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.default_solver(lsq.Cholesky(), K)
    assert "nb + ng <= 64" in str(e.value) and "nb = 60, ng = 5" in str(e.value) and "LSMR()" in str(e.value)
    assert isinstance(lsq.default_solver(lsq.LSMR(), K), lsq.LSMR)
    assert isinstance(lsq.default_solver(lsq.Cholesky(), lsq.BorderedBlockDiagonal(2, 70, 60, 4)), lsq.Cholesky)
    # optimize_: every refusal comes before anything reaches a device
    for opt in (lsq.Dogleg(lsq.QR()), lsq.LevenbergMarquardt(lsq.BlockQR()), lsq.LevenbergMarquardt(lsq.QR())):
        with pytest.raises(lsq.ArgumentError):
            lsq.optimize_(_problem(J), opt)
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.optimize_(_problem(K), lsq.LevenbergMarquardt(lsq.Cholesky()))
    assert "nb + ng <= 64" in str(e.value)
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.optimize_(_problem(J), lsq.Dogleg(lsq.Cholesky()))
    assert e.value.status == lsq._lib.EARG
    msg = str(e.value)
    assert "Dogleg(Cholesky()) is not available on a bordered" in msg
    assert "LevenbergMarquardt(Cholesky())" in msg and "LSMR()" in msg
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.default_optimizer(lsq.Dogleg(), lsq.Cholesky(), J)
    assert str(e.value) == msg
    for opt in (None, lsq.LevenbergMarquardt(lsq.Cholesky()), lsq.Dogleg(lsq.Cholesky())):
        with pytest.raises(lsq.ArgumentError) as e:
            lsq.optimize_batched_(_problem(J), opt)
        assert "BorderedBlockDiagonal" in str(e.value) and "optimize_" in str(e.value)


def test_new_entry_points_declared_and_exported():
    new = {"lsq_blockdiag_bordered_create": 6, "lsq_mat_bordered_info": 5}
    declared = lsq.declared_symbols()
    L = lsq.lib()
    for name, nargs in new.items():
        assert name in declared, name
        assert hasattr(L, name), name
        assert len(L._signatures[name][1]) == nargs


def test_bordered_inputs_are_the_dense_generator():
    B, mb, nb, ng = 3, 8, 2, 3
    v = lsq.synthetic.bordered_inputs(B, mb, nb, ng, 5)
    assert v.shape == (B * mb * (nb + ng),)
    assert np.array_equal(v[:B * mb * nb], lsq.synthetic.blockdiag_inputs(B, mb, nb, 5))
    J = lsq.BorderedBlockDiagonal(B, mb, nb, ng, data=v)
    assert np.array_equal(J.border.reshape(-1, order="F"), lsq.synthetic.dense_inputs(B * mb, ng, 6))
    assert 0.5 < np.std(J.border) * np.sqrt(B * mb) < 1.5          # N(0,1)/sqrt(m)
