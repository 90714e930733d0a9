"""Shared by the host and the GPU tier of the coloured central differences on general sparse patterns
(test_fd_sparse_host.py, test_p_gpu_fd_sparse.py): the patterns, row-wise models, special x values and the bit comparison.

ROW-WISE models: residual row i is computed from the x of ITS OWN pattern columns only (a CSR product, one sequential loop per
row, over elementwise polynomials in + and * -- correctly rounded operations whose result cannot depend on where an entry
stands in the vector).  So a row's value cannot change when a column outside its pattern is perturbed, which is the contract
of the colouring, and the coloured twin (all columns of a colour at once) and the dense twin (one column at a time) must
agree bit for bit on the stored positions."""
import numpy as np
import scipy.sparse as sp


def special_x(n, seed):
    """+-0, negative, |x| = 1e8 (relative step), 1e-300 (absolute step) among ordinary entries."""
    x = np.random.default_rng(seed).uniform(-2.0, 2.0, n)
    for k, v in enumerate((0.0, -0.0, -3.5, 1e8, 1e-300, -1e8)):
        if k < n:
            x[(k * 7) % n] = v
    return x


def same_bits(a, b, label=""):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, (label, a.shape, b.shape)
    bad = np.flatnonzero(a.view(np.uint64).reshape(-1) != b.view(np.uint64).reshape(-1))
    assert bad.size == 0, (label, bad.size, bad[:8], a.reshape(-1)[bad[:8]], b.reshape(-1)[bad[:8]])


def canonical(S):
    S = sp.csc_matrix(S, copy=True)
    S.sort_indices()
    S.data[:] = 1.0
    return S


def from_entries(m, n, rows, cols):
    return canonical(sp.coo_matrix((np.ones(len(rows)), (np.asarray(rows), np.asarray(cols))), shape=(m, n)))


# ------------------------------------------------------------------------------------------------ patterns
def blockdiag_pattern(B=5, mb=7, nb=3):
    return canonical(sp.block_diag([np.ones((mb, nb))] * B))


def band_pattern(n=40, w=4):
    """Row i holds columns i .. i+w-1."""
    m = n - w + 1
    return from_entries(m, n, np.repeat(np.arange(m), w), (np.arange(m)[:, None] + np.arange(w)[None, :]).reshape(-1))


def arrow_pattern(n=9):
    """A dense first row over an otherwise diagonal n x n."""
    return from_entries(n, n, np.concatenate([np.zeros(n, dtype=int), np.arange(1, n)]), np.concatenate([np.arange(n), np.arange(1, n)]))


def diagonal_pattern(n=7):
    return from_entries(n, n, np.arange(n), np.arange(n))


def holes_pattern():
    """Empty rows (2, 5, 9) and empty columns (0, 3, 6) among ordinary ones."""
    rows = [0, 1, 1, 3, 4, 4, 6, 7, 8, 8, 10, 10]
    cols = [1, 1, 2, 2, 4, 5, 5, 4, 1, 5, 2, 4]
    return from_entries(11, 7, rows, cols)


def random_pattern(seed, m=61, n=23, density=0.15):
    return canonical(sp.random(m, n, density, format="csc", random_state=np.random.default_rng(seed)))


def tall_column_pattern(m=3000, n=9):
    """One full column (column 4) beside columns of one or two entries: a long column that spans many workgroups, short
    columns that share rows with it only, and so a colour of one column."""
    rows = list(range(m)) + [0, 5, 17, 17, 100, 2999, 1500, 1501, 64, 65, 2048]
    cols = [4] * m + [0, 0, 1, 2, 3, 5, 6, 6, 7, 8, 8]
    return from_entries(m, n, rows, cols)


def permutation_pattern(n=2100, extra=30, seed=3):
    """A permutation pattern plus a few extra entries: more than 2000 columns in one colour."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    rows = np.concatenate([perm, rng.integers(0, n, extra)])
    cols = np.concatenate([np.arange(n), rng.integers(0, n, extra)])
    return from_entries(n, n, rows, cols)


def host_patterns():
    """name -> pattern: everything the host tier colours (the GPU tier differentiates on all of them too)."""
    P = {"blockdiag5x7x3": blockdiag_pattern(), "band40w4": band_pattern(), "arrow9": arrow_pattern(), "diag7": diagonal_pattern(),
         "holes11x7": holes_pattern(), "1x1": from_entries(1, 1, [0], [0]), "5x1": from_entries(5, 1, [0, 2, 4], [0, 0, 0]),
         "1x6": from_entries(1, 6, [0] * 6, list(range(6)))}
    for seed in range(5):
        P["random61x23s%d" % seed] = random_pattern(seed)
    return P


def valid(S, colour):
    """No row holds two columns of one colour."""
    S = canonical(S).tocoo()
    key = S.row.astype(np.int64) * (int(np.max(colour, initial=0)) + 1) + np.asarray(colour)[S.col]
    return np.unique(key).size == key.size


def max_row_count(S):
    S = canonical(S)
    return int(np.max(np.bincount(S.indices, minlength=S.shape[0]), initial=0))


# ------------------------------------------------------------------------------------------------ models
def poly_rowwise_model(S, seed):
    """r = A g(x) + (B x) .* (D x) with g(x) = x (1 + x) elementwise and A, B, D random values on the CSR view of the
    pattern: + and * only, every row from its own columns."""
    rng = np.random.default_rng(seed)
    R = canonical(S).tocsr()
    R.sort_indices()
    A, B, D = (sp.csr_matrix((rng.standard_normal(R.nnz), R.indices, R.indptr), shape=R.shape) for _ in range(3))

    def f_(out, x):
        out[:] = A @ (x * (1.0 + x)) + (B @ x) * (D @ x)

    return f_


def tanh_fit_problem(S, seed, noise=0.01):
    """A fit on the pattern: r = A tanh(x) - y, y = A tanh(x_true) + noise.  (f_, analytic values in CSC order as a function of
    x, x0, x_true)."""
    rng = np.random.default_rng(seed)
    C = canonical(S)
    C.data[:] = rng.uniform(0.5, 1.5, C.nnz) * rng.choice([-1.0, 1.0], C.nnz)
    R = C.tocsr()
    n = C.shape[1]
    x_true = rng.uniform(-0.8, 0.8, n)
    y = R @ np.tanh(x_true) + noise * rng.standard_normal(C.shape[0])
    x0 = x_true + 0.3 * rng.uniform(-1.0, 1.0, n)
    col_of = np.repeat(np.arange(n), np.diff(C.indptr))

    def f_(out, x):
        out[:] = R @ np.tanh(x) - y

    def values(x):
        return C.data * (1.0 - np.tanh(x) ** 2)[col_of]

    return f_, values, x0, x_true
