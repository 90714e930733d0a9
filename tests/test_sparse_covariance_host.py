"""Host tier of lsq_sparse_gram / lsq_sparse_covariance (no device): what tests/test_q_gpu_sparse_covariance.py relies on.
    * every operand of tests/sparse_cov_common.py has rank n;
    * numpy's fp64 inv(A.T @ A) (the e_ref of the rule) and the fp64 stand-in of the device algorithm behind the Gram matrix
      (ac.standin_inv) on the densified operand both stay inside the rule at every shape and family the GPU tier uses;
    * the plain Python twin of k_sp_gram -- the sums in the order of the column's stored entries, a product and an add per
      term -- meets the product bound per entry, and is exact on the integer-valued patterns;
    * the constants the GPU tier takes from the kernel's geometry, and the interface.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import accuracy_common as ac
import hp_reference as hp
import lsq_amd as lsq
import sparse_cov_common as sc


@pytest.mark.parametrize("m,n,family", sc.CASES)
def test_operands_have_full_rank_and_references_obey_the_rule(m, n, family):
    op, ref = sc.case(family, m, n)
    A = op.S.toarray()
    assert A.shape == (m, n) and sp.issparse(op.S) and op.S.has_sorted_indices
    norms = np.sqrt(np.sum(A * A, axis=0))
    assert np.all(norms > 0)
    assert np.linalg.matrix_rank(A / norms) == n                 # (normalised: the grading is not a rank defect)
    if n >= 2 and family != "ill":
        assert op.S.nnz < m * n                                  # it IS sparse
    stand = ac.standin_inv(A)
    pieces = ac.cov_pieces("numpy", ref.R, np.sqrt(np.diag(ref.R)), ref.R, ref.H, n)
    pieces += ac.cov_pieces("stand-in", stand, np.sqrt(np.diag(stand)), ref.R, ref.H, n)
    ac.judge("sparse covariance references %s %dx%d" % (family, m, n), pieces)
    if family == "graded":                                       # the column-scaled handle means V diag(s), unrounded
        eff = hp.ld(op.V.toarray()) * hp.ld(op.s)
        assert np.max(np.abs(eff - hp.ld(A)) / np.maximum(np.abs(eff), 1e-300)) <= ac.UNIT


def special_patterns():
    rng = np.random.default_rng(11)
    full = sp.random(40, 200, density=0.03, format="lil", random_state=rng, data_rvs=rng.standard_normal)
    full[7, :] = rng.standard_normal(200)
    long_col = sp.lil_matrix((3000, 6))
    long_col[:, 2] = rng.standard_normal((3000, 1))
    for i, j in ((0, 0), (5, 1), (9, 1), (17, 3), (2999, 4), (1500, 5), (1501, 5)):
        long_col[i, j] = rng.standard_normal()
    return {"1x1": sp.csc_matrix(np.array([[1.7]])), "5x1": sp.csc_matrix(rng.standard_normal((5, 1))),
            "1x6": sp.csc_matrix(rng.standard_normal((1, 6))), "ragged 300x65": ac.ragged_pattern(300, 65, 0.05, 3),
            "full row 40x200": full.tocsc(), "long column 3000x6": long_col.tocsc()}


@pytest.mark.parametrize("name", list(special_patterns()))
def test_twin_meets_the_product_bound(name):
    S = special_patterns()[name]
    m, n = S.shape
    # (the column factors of ac.product_scales; ac.grading has no n = 1 or m = 1)
    c = np.random.default_rng(5).permutation(ac.grading(n, 12.0)) if n >= 2 else np.array([0.37])
    damp = 0.05 + np.random.default_rng(6).random(n)
    for label, cs, dp, extra in (("plain", None, None, 0), ("colscale", c, None, 2), ("damped", None, damp, 1)):
        G = sc.gram_twin(S, cs, dp)
        ref, mag, K = sc.gram_reference(S, cs, dp)
        q, at = sc.gram_excess(G, ref, mag, K, extra)
        print("twin %s %s: worst |err| / bound %.3f at %s" % (name, label, q, at))
        assert q <= 1.0
        assert np.all(G[np.tril_indices(n, -1)] == 0)
        if dp is None:
            assert np.all(G[(K == 0) & np.triu(np.ones((n, n), bool))] == 0)


def test_twin_is_exact_on_integer_patterns():
    for m, n in ((70, 64), (131, 130)):
        S = sc.band_int(m, n, 3)
        assert np.max(np.diff(S.tocsr().indptr)) <= 3
        assert np.array_equal(sc.gram_twin(S), np.triu((S.T @ S).toarray()))
    S, _ = sc.block_pattern(5, 12, 8, 4)
    Si = sp.csc_matrix(np.round(4 * S.toarray()))
    assert np.array_equal(sc.gram_twin(Si), np.triu((Si.T @ Si).toarray()))


def test_geometry_constants():
    """The n on either side of each change of W, as the GPU tier uses them, and the limit."""
    assert [sc.gram_waves(n) for n in (1, 5120, 5121, 6826, 6827, 10240, 10241, sc.GRAM_MAX_N)] == [4, 4, 3, 3, 2, 2, 1, 1]
    for lo, hi in sc.W_SWITCHES:
        assert sc.gram_waves(lo) == sc.gram_waves(hi) + 1
    assert sc.gram_waves(sc.GRAM_MAX_N) * 8 * sc.GRAM_MAX_N <= sc.GRAM_LDS_BUDGET
    src = open(lsq._lib.ROOT + "/leastsquaresoptim.jl_amd/csrc/lsq_cov_sparse.hip").read()
    assert "SG_MAX_N = %d;" % sc.GRAM_MAX_N in src and "SG_LDS_BUDGET = 160 * 1024;" in src and "SG_MAX_WAVES = 4;" in src


def test_interface():
    declared = lsq.declared_symbols()
    assert "lsq_sparse_gram" in declared and "lsq_sparse_covariance" in declared
    if lsq._lib.os.path.exists(lsq._lib.LIB_PATH):
        L = lsq.lib()
        assert len(L._signatures["lsq_sparse_gram"][1]) == 3
        assert L._signatures["lsq_sparse_covariance"] == L._signatures["lsq_dense_covariance"]     # argument for argument
    assert callable(lsq.sparse_covariance) and callable(lsq.sparse_gram)
    assert hasattr(lsq.AllocatedSolver, "sparse_covariance")
    d = lsq.DenseCovariance(2, None, np.ones(2), chol_path="blocked")
    assert d.cov is None and d.chol_path == "blocked" and d.stderr.shape == (2,)
    assert lsq.DenseCovariance(2, np.eye(2)).chol_path is None
