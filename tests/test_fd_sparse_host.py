"""Host tier of the coloured central differences on general sparse patterns (csrc/lsq_fd.hip, api.py): the greedy colouring
through the C entry against its Python twin and against expectations that can be proved for first fit in natural order, the
host twin of the device routine against the dense twin, and the wiring of autodiff="central_coloured".  No GPU."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import lsq_amd as lsq
from lsq_amd import api

import fd_sparse_common as FS

L_ = lsq._lib
PATTERNS = FS.host_patterns()


# ------------------------------------------------------------------------------------------------ 1. the greedy colouring
def test_symbols_declared_and_bound():
    import julia_shim_lint as JL
    protos = JL.header_prototypes()
    assert protos["lsq_csc_greedy_colouring"] == ("int", ["int", "int", "ptr:int", "ptr:int", "ptr:int", "ptr:int"])
    assert protos["lsq_mat_set_fd_colouring"] == ("int", ["ptr:void", "ptr:int", "ptr:int"])
    assert protos["lsq_mat_fd_colouring"] == ("int", ["ptr:void", "ptr:int", "ptr:int"])
    shim = {c[0] for c in JL.ccalls()}
    assert {"lsq_csc_greedy_colouring", "lsq_mat_set_fd_colouring", "lsq_mat_fd_colouring"} <= shim


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_greedy_colouring_c_entry_equals_python_twin(name):
    S = PATTERNS[name]
    colour, nc = lsq.greedy_colouring(S)
    twin, nct = api._greedy_colouring_host(S)
    assert colour.dtype == np.int32 and colour.shape == (S.shape[1],)
    assert np.array_equal(colour, twin) and nc == nct
    assert nc == int(colour.max()) + 1 and colour.min() >= 0
    assert set(colour.tolist()) == set(range(nc))                  # no gap
    assert FS.valid(S, colour)
    assert nc >= max(FS.max_row_count(S), 1)                       # the longest row is a lower bound
    empty = np.flatnonzero(np.diff(S.indptr) == 0)
    assert np.all(colour[empty] == 0)


def test_greedy_colouring_exact_expectations():
    colour, nc = lsq.greedy_colouring(PATTERNS["blockdiag5x7x3"])
    assert np.array_equal(colour, np.arange(15) % 3) and nc == 3
    colour, nc = lsq.greedy_colouring(PATTERNS["band40w4"])
    assert np.array_equal(colour, np.arange(40) % 4) and nc == 4
    colour, nc = lsq.greedy_colouring(PATTERNS["arrow9"])
    assert np.array_equal(colour, np.arange(9)) and nc == 9
    colour, nc = lsq.greedy_colouring(PATTERNS["diag7"])
    assert np.array_equal(colour, np.zeros(7)) and nc == 1
    assert lsq.greedy_colouring(PATTERNS["1x1"])[1] == 1
    assert lsq.greedy_colouring(PATTERNS["5x1"])[1] == 1
    colour, nc = lsq.greedy_colouring(PATTERNS["1x6"])
    assert np.array_equal(colour, np.arange(6)) and nc == 6


def test_greedy_colouring_pattern_errors():
    """LSQ_EDIM / LSQ_EARG as lsq_csc_create reports them."""
    ip = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(L_.c_ip)
    out, nc = np.zeros(4, dtype=np.int32), C.c_int(0)
    call = lambda m, n, colptr, rowval: lsq.lib().lsq_csc_greedy_colouring(m, n, ip(colptr), ip(rowval), out.ctypes.data_as(L_.c_ip),
                                                                          C.byref(nc))
    assert call(3, 2, [0, 1, 2], [0, 2]) == L_.OK
    assert call(3, 2, [1, 1, 2], [0, 2]) == L_.EDIM                 # colptr does not start at 0
    assert call(3, 2, [0, 2, 1], [0, 2]) == L_.EDIM                 # not monotone
    assert call(3, 2, [0, 1, 2], [0, 3]) == L_.EDIM                 # row out of range
    assert call(3, 2, [0, 1, 2], [-1, 1]) == L_.EDIM
    assert call(-1, 2, [0, 1, 2], [0, 1]) == L_.EARG
    assert lsq.lib().lsq_csc_greedy_colouring(3, 2, None, None, out.ctypes.data_as(L_.c_ip), C.byref(nc)) == L_.EARG


# ------------------------------------------------------------------------------------------------ 2. the host twin
def hand_made_colouring(S):
    """Valid, and neither the greedy nor the trivial one: the greedy colours relabelled in reverse."""
    colour, nc = lsq.greedy_colouring(S)
    return (nc - 1 - colour).astype(np.int32)


@pytest.mark.parametrize("which", ["greedy", "trivial", "hand"])
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_twin_equals_dense_twin_on_the_pattern(name, which):
    S = PATTERNS[name]
    m, n = S.shape
    colour = {"greedy": lambda: lsq.greedy_colouring(S)[0], "trivial": lambda: np.arange(n, dtype=np.int32),
              "hand": lambda: hand_made_colouring(S)}[which]()
    assert FS.valid(S, colour)
    f_ = FS.poly_rowwise_model(S, 11)
    x = FS.special_x(n, 5)
    J = S.copy()
    J.data[:] = np.nan
    calls = []

    def counted(out, xx):
        calls.append(xx.copy())
        f_(out, xx)

    api._sparse_colored_difference_jacobian(counted, m, colour)(J, x)
    assert len(calls) == 2 * (int(colour.max()) + 1)
    D = np.full((m, n), np.nan, order="F")
    api._central_difference_jacobian(f_, m)(D, x)
    mask = S.toarray() != 0
    assert np.all(np.isfinite(J.data))
    coo = J.tocoo()
    FS.same_bits(coo.data, D[coo.row, coo.col], (name, which))          # bit for bit on the stored positions
    assert np.all(D[~mask] == 0.0)                                      # and the dense twin finds exactly 0 elsewhere
    # the calls: colour by colour, f+ then f-, full vectors that differ from x in that colour's columns only
    for c in range(int(colour.max()) + 1):
        for v in calls[2 * c:2 * c + 2]:
            assert np.array_equal(np.flatnonzero(v.view(np.uint64) != x.view(np.uint64)), np.flatnonzero(colour == c))


def test_twin_with_a_superfluous_entry_gives_zero():
    S = FS.diagonal_pattern(5)
    wide = FS.from_entries(5, 5, [0, 1, 2, 3, 4, 0], [0, 1, 2, 3, 4, 3])       # (0, 3) is stored, f_ does not depend on it
    f_ = FS.poly_rowwise_model(S, 2)
    J = wide.copy()
    api._sparse_colored_difference_jacobian(f_, 5, lsq.greedy_colouring(wide)[0])(J, FS.special_x(5, 1))
    assert J[0, 3] == 0.0 and np.all(J.diagonal() != 0.0)


# ------------------------------------------------------------------------------------------------ 3. LeastSquaresProblem
def test_problem_wiring():
    S = PATTERNS["random61x23s1"]
    m, n = S.shape
    f_ = FS.poly_rowwise_model(S, 4)
    x = FS.special_x(n, 6)
    nls = lsq.LeastSquaresProblem(x=x, y=np.zeros(m), f_=f_, J=S.copy(), autodiff="central_coloured")
    assert api._device_fd(nls)
    assert np.array_equal(nls._fd_colouring, lsq.greedy_colouring(S)[0])
    nls.g_(nls.J, nls.x)
    ref = S.copy()
    api._sparse_colored_difference_jacobian(f_, m, lsq.greedy_colouring(S)[0])(ref, x)
    FS.same_bits(nls.J.data, ref.data)
    # a colouring of the caller's
    hand = hand_made_colouring(S)
    nls2 = lsq.LeastSquaresProblem(x=x, y=np.zeros(m), f_=f_, J=S.copy(), autodiff="central_coloured", colouring=hand)
    assert api._device_fd(nls2) and np.array_equal(nls2._fd_colouring, hand)
    nls2.g_(nls2.J, nls2.x)
    FS.same_bits(nls2.J.data, ref.data)
    # a g_ of the user's own ends it
    nls.g_ = lambda Jm, xx: None
    assert not api._device_fd(nls)
    given = lsq.LeastSquaresProblem(x=x, y=np.zeros(m), f_=f_, g_=lambda Jm, xx: None, J=S.copy(), autodiff="central_coloured")
    assert not api._device_fd(given)


def test_problem_refusals():
    S = PATTERNS["arrow9"]
    f_ = FS.poly_rowwise_model(S, 4)
    make = lambda **kw: lsq.LeastSquaresProblem(x=np.ones(9), y=np.zeros(9), f_=f_, **kw)
    bad = np.arange(9, dtype=np.int32)
    bad[5] = 2                                           # columns 2 and 5 meet in row 0 (and colour 5 is unused)
    with pytest.raises(lsq.ArgumentError):
        make(J=S.copy(), autodiff="central_coloured", colouring=bad)
    clash = np.arange(9, dtype=np.int32)
    clash[[2, 5]] = [5, 5]
    clash[8] = 2                                         # no gap, every value >= 0: only the clash in row 0 is wrong
    with pytest.raises(lsq.ArgumentError, match="row 0 .*columns 2 and 5"):
        make(J=S.copy(), autodiff="central_coloured", colouring=clash)
    with pytest.raises(lsq.ArgumentError):
        make(J=S.copy(), autodiff="central_coloured", colouring=-np.arange(9))
    with pytest.raises(lsq.ArgumentError):
        make(J=S.copy(), autodiff="central_coloured", colouring=np.arange(9) * 2)          # gaps
    with pytest.raises(lsq.ArgumentError):
        make(J=S.copy(), autodiff="central_coloured", colouring=np.arange(8))              # wrong length
    with pytest.raises(lsq.ArgumentError):
        make(J=np.zeros((9, 9)), autodiff="central_coloured")                              # a dense J
    with pytest.raises(lsq.ArgumentError):
        make(J=lsq.BlockDiagonal(3, 3, 3), autodiff="central_coloured")
    # autodiff="central" with a sparse J keeps raising at the first g!
    nls = make(J=S.copy())
    assert not api._device_fd(nls)
    with pytest.raises(lsq.ArgumentError):
        nls.g_(nls.J, nls.x)
