"""Block-diagonal Jacobians, host tier (no device): the BlockDiagonal container, the solver / optimizer defaults on it and
the three C entry points (lsq_blockdiag_create, lsq_mat_blockdiag_info, lsq_solver_blockdiag_path) in header, loader and
library."""
import numpy as np
import pytest

import lsq_amd as lsq


def _random_blocks(B, mb, nb, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((mb, nb)) for _ in range(B)]


@pytest.mark.parametrize("B,mb,nb", [(1, 1, 1), (3, 5, 2), (4, 2, 6), (7, 9, 9)])
def test_layout_is_the_csc_layout(B, mb, nb):
    blocks = _random_blocks(B, mb, nb, 10 * B + nb)
    J = lsq.BlockDiagonal.from_blocks(blocks)
    assert (J.nblocks, J.mb, J.nb) == (B, mb, nb)
    assert J.shape == (B * mb, B * nb) and J.nnz == B * mb * nb == J.data.size
    # [block][column][row]: B column-major blocks back to back
    assert np.array_equal(J.data, np.concatenate([b.reshape(-1, order="F") for b in blocks]))
    S = J.tocsc()
    assert S.shape == J.shape and S.nnz == J.nnz and S.has_sorted_indices
    assert np.array_equal(S.data, J.data)              # the nzval order of the equivalent sparse matrix
    dense = np.zeros(J.shape)
    for b, blk in enumerate(blocks):
        dense[b * mb:(b + 1) * mb, b * nb:(b + 1) * nb] = blk
    assert np.array_equal(S.toarray(), dense) and np.array_equal(J.toarray(), dense)
    assert S.data is not J.data                        # (a copy: the scipy matrix is not a view of the container)


def test_block_is_a_view_and_round_trip():
    blocks = _random_blocks(5, 4, 3, 1)
    J = lsq.BlockDiagonal.from_blocks(blocks)
    for b, blk in enumerate(blocks):
        assert np.array_equal(J.block(b), blk)
    v = J.block(2)
    assert np.shares_memory(v, J.data) and v.shape == (4, 3)
    v[1, 2] = 77.0
    assert J.data[2 * 12 + 2 * 4 + 1] == 77.0
    J.data[0] = -5.0
    assert J.block(0)[0, 0] == -5.0
    # g! may rebind .data (optimize_ hands it a page-locked array): block() follows the binding
    J.data = np.arange(J.nnz, dtype=np.float64)
    assert J.block(1)[0, 0] == 12.0 and J.block(4)[3, 2] == J.nnz - 1
    # explicit data
    K = lsq.BlockDiagonal(5, 4, 3, data=J.data)
    assert np.array_equal(K.toarray(), J.toarray())
    Z = lsq.BlockDiagonal(2, 3, 2)
    assert Z.data.shape == (12,) and not Z.data.any()


def test_dimension_errors():
    with pytest.raises(lsq.DimensionMismatch):
        lsq.BlockDiagonal(0, 3, 2)
    with pytest.raises(lsq.DimensionMismatch):
        lsq.BlockDiagonal(2, 0, 2)
    with pytest.raises(lsq.DimensionMismatch):
        lsq.BlockDiagonal(2, 3, -1)
    with pytest.raises(lsq.DimensionMismatch):
        lsq.BlockDiagonal(2, 3, 2, data=np.zeros(11))
    with pytest.raises(lsq.DimensionMismatch):
        lsq.BlockDiagonal.from_blocks([np.zeros((3, 2)), np.zeros((2, 3))])
    with pytest.raises(lsq.DimensionMismatch):
        lsq.BlockDiagonal.from_blocks([])
    with pytest.raises(IndexError):
        lsq.BlockDiagonal(2, 3, 2).block(2)
    J = lsq.BlockDiagonal(2, 3, 2)
    f_ = lambda out, x: None
    with pytest.raises(lsq.DimensionMismatch):
        lsq.LeastSquaresProblem(x=np.zeros(5), y=np.zeros(6), f_=f_, g_=lambda J, x: None, J=J)
    with pytest.raises(lsq.DimensionMismatch):
        lsq.LeastSquaresProblem(x=np.zeros(4), y=np.zeros(7), f_=f_, g_=lambda J, x: None, J=J)
    nls = lsq.LeastSquaresProblem(x=np.zeros(4), f_=f_, g_=lambda J, x: None, J=J)
    assert nls.J is J and len(nls.y) == 6           # output_length = size(J, 1); the container is kept, not converted


def test_default_solver_and_optimizer():
    J = lsq.BlockDiagonal(3, 4, 2)
    s = lsq.default_solver(None, J)
    assert isinstance(s, lsq.LSMR)                                  # types.jl:114-127: anything not dense
    assert isinstance(lsq.default_optimizer(None, s), lsq.LevenbergMarquardt)
    c = lsq.default_solver(lsq.Cholesky(), J)
    assert isinstance(c, lsq.Cholesky)                              # what the user asks for explicitly
    assert isinstance(lsq.default_optimizer(None, c), lsq.Dogleg)
    assert isinstance(lsq.default_optimizer(lsq.LevenbergMarquardt(), c), lsq.LevenbergMarquardt)
    with pytest.raises(lsq.ArgumentError) as e:
        lsq.default_solver(lsq.QR(), J)
    assert "Cholesky()" in str(e.value) and "LSMR()" in str(e.value)


def test_new_entry_points_declared_and_exported():
    new = ["lsq_blockdiag_create", "lsq_mat_blockdiag_info", "lsq_solver_blockdiag_path"]
    declared = lsq.declared_symbols()
    for name in new:
        assert name in declared, name
    L = lsq.lib()
    for name in new:
        assert hasattr(L, name), name
        assert name in L._signatures, name
    assert len(L._signatures["lsq_blockdiag_create"][1]) == 5
    assert len(L._signatures["lsq_mat_blockdiag_info"][1]) == 4
    assert len(L._signatures["lsq_solver_blockdiag_path"][1]) == 3


def test_blockdiag_inputs_are_the_dense_generator():
    B, mb, nb = 3, 8, 2
    v = lsq.synthetic.blockdiag_inputs(B, mb, nb, 5)
    assert v.shape == (B * mb * nb,)
    assert np.array_equal(v, lsq.synthetic.dense_inputs(mb, B * nb, 5))
    J = lsq.BlockDiagonal(B, mb, nb, data=v)
    assert np.array_equal(J.block(1), v.reshape((mb, B * nb), order="F")[:, nb:2 * nb])
