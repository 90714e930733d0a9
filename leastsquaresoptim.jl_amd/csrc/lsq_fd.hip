// Central-difference Jacobians on the device (types.jl:54-58: the reference's default problem has no g!, its closure
// differentiates f! by central differences).  Dense, block-diagonal and bordered block-diagonal handles; the values go
// straight into lsq_mat_values(J).
//
// The columns split into COLOURS, sets of columns no residual row depends on two of: a dense m x n handle has n colours of one
// column; on a block-diagonal handle column c of EVERY block is one colour (nb colours, whatever B is); a bordered handle has
// those nb and then one per shared column.  One description covers the three: B blocks of mb x nb followed by ng full columns
// (dense: B = 1, mb = m, nb = 0, ng = n).
//
// Per colour the stream carries f!(f+, x+), f!(f-, x-) and ONE launch of the library, k_fd_step, which writes the colour's
// column(s) from f+ - f- and moves the two work vectors x+ / x- on to the next colour (only the entries of the two colours are
// touched); k_fd_begin in front makes x+ / x- from x with colour 0 set.  colours + 1 launches per Jacobian, 24 bytes per entry.
//
// The step of entry j is h = max(eps3 |x_j|, eps3); x_j + h and x_j - h are formed from x itself (never from a perturbed
// copy), and the store kernel forms h again from x by the same expression: the column is (f+ - f-) / (2 h), one correctly
// rounded operation each (-ffp-contract=off), the bits of the host twin (api.py).  Everything is stream order: no atomics,
// no exchange between workgroups, no waits.
//
// A plain CSC handle has no colouring of its own: it takes central differences once one is attached to it
// (lsq_mat_set_fd_colouring: the first-fit colouring of lsq_csc_greedy_colouring, or the caller's, validated).  The stream has
// the same shape -- k_fd_sparse_begin in front, then per colour f!, f! and ONE launch, k_fd_sparse_step -- but the store is
// balanced by STORED ENTRIES, not by columns: the columns are kept sorted by colour (cols) with the running entry count in
// that order (off); a thread takes flat entry t of the colour, finds its column by a binary search of off inside the colour's
// range (a few KB, cache-resident), reads the row index, gathers f+ / f- and stores into nzval.  Entries of one column are
// contiguous in nzval, so the stores coalesce; every stored entry is written exactly once per Jacobian by exactly one thread.
// 28 bytes per stored entry (4 row index + 16 gathered + 8 stored) plus O(n) per colour.
#include <algorithm>
#include <cstdint>
#include <new>
#include <vector>

#include "lsq_common.h"

namespace {

// numpy.finfo(float).eps ** (1/3), the constant of the host twin -- NOT cbrt(DBL_EPSILON), which ends in ...e3d
constexpr double FD_EPS3 = 0x1.965fea53d6e41p-18;

struct FdShape {
    int B, mb, nb, ng, m;     // m = B * mb; colours 0 .. nb-1 are the block columns, nb .. nb+ng-1 the full columns
};

// max(eps3 * abs(x), eps3) as Python evaluates it: the second operand only if it is greater (a NaN x gives a NaN step)
__device__ __forceinline__ double fd_h(double xj) {
    const double a = FD_EPS3 * fabs(xj);
    return FD_EPS3 > a ? FD_EPS3 : a;
}

// entries of colour q: t < fd_count(q) -> fd_entry(q, t)
__device__ __forceinline__ int fd_count(const FdShape &s, int q) { return q < 0 ? 0 : (q < s.nb ? s.B : 1); }
__device__ __forceinline__ size_t fd_entry(const FdShape &s, int q, int t) {
    return q < s.nb ? (size_t)t * s.nb + q : (size_t)s.B * s.nb + (q - s.nb);
}

// x+ = x- = x with colour 0 set
__global__ void __launch_bounds__(LSQ_NT)
k_fd_begin(FdShape s, int n, const double *__restrict__ x, double *__restrict__ xp, double *__restrict__ xm) {
    const int nloc = s.B * s.nb;
    for (long long i = blockIdx.x * (long long)LSQ_NT + threadIdx.x; i < n; i += (long long)gridDim.x * LSQ_NT) {
        const double xi = x[i];
        const bool hit = s.nb > 0 ? (i < nloc && i % s.nb == 0) : i == 0;
        const double h = hit ? fd_h(xi) : 0.0;
        xp[i] = hit ? xi + h : xi;
        xm[i] = hit ? xi - h : xi;
    }
}

// store colour c, then x+ / x- : colour c back to x, colour cn (-1: none) set.  V2: two rows per access (mb even, 16-byte
// aligned pointers: a pair of rows never straddles a block); else one row (a block's column start is 8-byte aligned only).
template <bool V2>
__global__ void __launch_bounds__(LSQ_NT)
k_fd_step(FdShape s, int c, int cn, const double *__restrict__ x, double *__restrict__ xp, double *__restrict__ xm,
          const double *__restrict__ fp, const double *__restrict__ fm, double *__restrict__ vals) {
    const int tid = blockIdx.x * LSQ_NT + threadIdx.x, nth = gridDim.x * LSQ_NT;
    const int cnt_c = fd_count(s, c), cnt_n = fd_count(s, cn);
    for (long long t = tid; t < cnt_c || t < cnt_n; t += nth) {
        if (t < cnt_c) {
            const size_t j = fd_entry(s, c, (int)t);
            const double xj = x[j];
            xp[j] = xj;
            xm[j] = xj;
        }
        if (t < cnt_n) {
            const size_t j = fd_entry(s, cn, (int)t);
            const double xj = x[j], h = fd_h(xj);
            xp[j] = xj + h;
            xm[j] = xj - h;
        }
    }
    constexpr int W = V2 ? 2 : 1;
    const int work = s.m / W;
    const bool local = c < s.nb;
    const size_t border0 = (size_t)s.B * s.mb * s.nb + (size_t)(local ? 0 : c - s.nb) * s.m;
    const double xg = local ? 0.0 : x[(size_t)s.B * s.nb + (c - s.nb)];
#pragma unroll 2
    for (long long q = tid; q < work; q += nth) {
        const int r = (int)q * W;
        double xj = xg;
        size_t dst = border0 + r;
        if (local) {
            const int b = r / s.mb;
            xj = x[(size_t)b * s.nb + c];
            dst = ((size_t)b * s.nb + c) * s.mb + (r - b * s.mb);
        }
        const double h2 = 2.0 * fd_h(xj);
        if (V2) {
            const double2 a = *reinterpret_cast<const double2 *>(fp + r), d = *reinterpret_cast<const double2 *>(fm + r);
            double2 o;
            o.x = (a.x - d.x) / h2;
            o.y = (a.y - d.y) / h2;
            *reinterpret_cast<double2 *>(vals + dst) = o;
        } else {
            vals[dst] = (fp[r] - fm[r]) / h2;
        }
    }
}

// ---- plain CSC handles with an attached colouring ------------------------------------------------------------------------
// x+ = x- = x with colour 0 set
__global__ void __launch_bounds__(LSQ_NT)
k_fd_sparse_begin(int n, const int *__restrict__ colour, const double *__restrict__ x, double *__restrict__ xp,
                  double *__restrict__ xm) {
    for (long long i = blockIdx.x * (long long)LSQ_NT + threadIdx.x; i < n; i += (long long)gridDim.x * LSQ_NT) {
        const double xi = x[i];
        const bool hit = colour[i] == 0;
        const double h = hit ? fd_h(xi) : 0.0;
        xp[i] = hit ? xi + h : xi;
        xm[i] = hit ? xi - h : xi;
    }
}

// largest p in [lo, hi) with off[p] <= t, given off[lo] <= t < off[hi] (an empty column shares its offset with its successor
// and is never the answer)
__device__ __forceinline__ int fd_find(const int *__restrict__ off, int lo, int hi, int t) {
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The colour's columns are cols[b0 .. b1) and its stored entries the flat range [e0, e1) = [off[b0], off[b1]); the next
// colour's columns are cols[b1 .. b2) (b2 == b1: none).  x+ / x-: this colour back to x, the next one set; then every stored
// entry of this colour, one per thread and round.
__global__ void __launch_bounds__(LSQ_NT)
k_fd_sparse_step(int b0, int b1, int b2, int e0, int e1, const int *__restrict__ cols, const int *__restrict__ off,
                 const int *__restrict__ colptr, const int *__restrict__ rowval, const double *__restrict__ x,
                 double *__restrict__ xp, double *__restrict__ xm, const double *__restrict__ fp, const double *__restrict__ fm,
                 double *__restrict__ vals) {
    const long long tid = blockIdx.x * (long long)LSQ_NT + threadIdx.x, nth = (long long)gridDim.x * LSQ_NT;
    const int cnt_c = b1 - b0, cnt_n = b2 - b1;
    for (long long t = tid; t < cnt_c || t < cnt_n; t += nth) {
        if (t < cnt_c) {
            const int j = cols[b0 + t];
            const double xj = x[j];
            xp[j] = xj;
            xm[j] = xj;
        }
        if (t < cnt_n) {
            const int j = cols[b1 + t];
            const double xj = x[j], h = fd_h(xj);
            xp[j] = xj + h;
            xm[j] = xj - h;
        }
    }
#pragma unroll 2
    for (long long t = e0 + tid; t < e1; t += nth) {
        const int p = fd_find(off, b0, b1, (int)t);
        const int j = cols[p];
        const int k = colptr[j] + ((int)t - off[p]);
        const int i = rowval[k];
        const double h2 = 2.0 * fd_h(x[j]);
        vals[k] = (fp[i] - fm[i]) / h2;
    }
}

bool fd_aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

// ---- host side of the colouring ------------------------------------------------------------------------------------------
// the pattern checks of lsq_csc_create
int fd_check_pattern(const char *who, int m, int n, const int *colptr, const int *rowval) {
    if (m < 0 || n < 0 || !colptr) {
        lsq_set_error("%s: bad arguments", who);
        return LSQ_EARG;
    }
    const long long nnz = colptr[n];
    if (colptr[0] != 0 || nnz < 0 || nnz > 2147483000LL) {
        lsq_set_error("%s: colptr must start at 0 and nnz must fit int32", who);
        return LSQ_EDIM;
    }
    for (int j = 0; j < n; ++j)
        if (colptr[j + 1] < colptr[j]) {
            lsq_set_error("%s: colptr not monotone at column %d", who, j);
            return LSQ_EDIM;
        }
    if (nnz > 0 && !rowval) {
        lsq_set_error("%s: bad arguments", who);
        return LSQ_EARG;
    }
    for (long long k = 0; k < nnz; ++k)
        if (rowval[k] < 0 || rowval[k] >= m) {
            lsq_set_error("%s: row index out of range at entry %lld", who, k);
            return LSQ_EDIM;
        }
    return LSQ_OK;
}

// row view of the pattern by counting sort: the columns of a row come out in increasing order
void fd_row_view(int m, int n, const int *colptr, const int *rowval, std::vector<int> &rptr, std::vector<int> &ridx) {
    const int nnz = colptr[n];
    rptr.assign((size_t)m + 1, 0);
    ridx.resize((size_t)nnz);
    for (int k = 0; k < nnz; ++k) rptr[rowval[k] + 1]++;
    for (int i = 0; i < m; ++i) rptr[i + 1] += rptr[i];
    std::vector<int> fill(rptr.begin(), rptr.end() - 1);
    for (int j = 0; j < n; ++j)
        for (int k = colptr[j]; k < colptr[j + 1]; ++k) ridx[fill[rowval[k]]++] = j;
}

// first fit in natural column order; stamp[c] == j: colour c is taken by an earlier column that shares a row with j
int fd_greedy(int m, int n, const int *colptr, const int *rowval, int *colour) {
    std::vector<int> rptr, ridx;
    fd_row_view(m, n, colptr, rowval, rptr, ridx);
    std::vector<int> stamp((size_t)n + 1, -1);
    int ncolours = 0;
    for (int j = 0; j < n; ++j) {
        for (int k = colptr[j]; k < colptr[j + 1]; ++k) {
            const int i = rowval[k];
            for (int q = rptr[i]; q < rptr[i + 1] && ridx[q] < j; ++q) stamp[colour[ridx[q]]] = j;
        }
        int c = 0;
        while (stamp[c] == j) ++c;       // (at most j earlier columns: stamp[j] is never taken)
        colour[j] = c;
        ncolours = std::max(ncolours, c + 1);
    }
    return ncolours;
}

// a caller's colouring: every value >= 0, every value 0 .. max used, no row with two columns of one colour.  O(nnz + n)
int fd_validate(int m, int n, const int *colptr, const int *rowval, const int *colour, int *ncolours) {
    int maxc = -1;
    for (int j = 0; j < n; ++j) {
        if (colour[j] < 0) {
            lsq_set_error("lsq_mat_set_fd_colouring: column %d has the negative colour %d", j, colour[j]);
            return LSQ_EARG;
        }
        if (colour[j] >= n) {
            lsq_set_error("lsq_mat_set_fd_colouring: column %d has colour %d, but %d columns cannot use every colour 0 .. %d "
                          "(the colours must be 0 .. ncolours-1 without a gap)", j, colour[j], n, colour[j]);
            return LSQ_EARG;
        }
        maxc = std::max(maxc, colour[j]);
    }
    std::vector<int> used((size_t)maxc + 1, 0);
    for (int j = 0; j < n; ++j) used[colour[j]]++;
    for (int c = 0; c <= maxc; ++c)
        if (!used[c]) {
            lsq_set_error("lsq_mat_set_fd_colouring: no column has colour %d although colour %d is used (the colours must be "
                          "0 .. ncolours-1 without a gap)", c, maxc);
            return LSQ_EARG;
        }
    std::vector<int> rptr, ridx;
    fd_row_view(m, n, colptr, rowval, rptr, ridx);
    std::vector<int> stamp((size_t)maxc + 1, -1), who((size_t)maxc + 1, -1);
    for (int i = 0; i < m; ++i)
        for (int q = rptr[i]; q < rptr[i + 1]; ++q) {
            const int j = ridx[q], c = colour[j];
            if (stamp[c] == i && who[c] != j) {
                lsq_set_error("lsq_mat_set_fd_colouring: row %d holds columns %d and %d, both of colour %d: their differences "
                              "would be added up in that row", i, who[c], j, c);
                return LSQ_EARG;
            }
            stamp[c] = i;
            who[c] = j;
        }
    *ncolours = maxc + 1;
    return LSQ_OK;
}

int fd_set_colouring_impl(lsq_mat *J, const int *h_colour, int *h_ncolours) {
    lsq_ctx *c = J->ctx;
    const int m = J->m, n = J->n;
    LSQ_HIP(hipSetDevice(c->device));
    std::vector<int> colptr((size_t)n + 1, 0), rowval((size_t)J->nnz);
    LSQ_HIP(hipMemcpy(colptr.data(), J->csc.d_ptr, ((size_t)n + 1) * sizeof(int), hipMemcpyDeviceToHost));
    if (J->nnz) LSQ_HIP(hipMemcpy(rowval.data(), J->csc.d_idx, (size_t)J->nnz * sizeof(int), hipMemcpyDeviceToHost));
    LsqFdColouring *fc = new LsqFdColouring();
    struct Guard {       // (an error below must not leak the tables)
        LsqFdColouring *p;
        ~Guard() {
            if (!p) return;
            hipFree(p->d_colour);
            hipFree(p->d_cols);
            hipFree(p->d_off);
            delete p;
        }
    } guard{fc};
    fc->colour.resize((size_t)n);
    if (h_colour) {
        LSQ_TRY(fd_validate(m, n, colptr.data(), rowval.data(), h_colour, &fc->ncolours));
        std::copy(h_colour, h_colour + n, fc->colour.begin());
    } else {
        fc->ncolours = fd_greedy(m, n, colptr.data(), rowval.data(), fc->colour.data());
    }
    const int nc = fc->ncolours;
    // the columns sorted by colour (counting sort: natural order inside a colour), the running entry count in that order
    fc->bound.assign((size_t)nc + 1, 0);
    for (int j = 0; j < n; ++j) fc->bound[fc->colour[j] + 1]++;
    for (int q = 0; q < nc; ++q) fc->bound[q + 1] += fc->bound[q];
    std::vector<int> cols((size_t)n), off((size_t)n + 1, 0);
    {
        std::vector<int> fill(fc->bound.begin(), fc->bound.end() - (nc > 0 ? 1 : 0));
        for (int j = 0; j < n; ++j) cols[fill[fc->colour[j]]++] = j;
    }
    for (int p = 0; p < n; ++p) off[p + 1] = off[p] + (colptr[cols[p] + 1] - colptr[cols[p]]);
    fc->ebound.resize((size_t)nc + 1);
    for (int q = 0; q <= nc; ++q) fc->ebound[q] = off[fc->bound[q]];
    const size_t nb = (size_t)std::max(n, 1) * sizeof(int);
    LSQ_HIP(hipMalloc(&fc->d_colour, nb));
    LSQ_HIP(hipMalloc(&fc->d_cols, nb));
    LSQ_HIP(hipMalloc(&fc->d_off, nb + sizeof(int)));
    if (n) {
        LSQ_HIP(hipMemcpy(fc->d_colour, fc->colour.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));
        LSQ_HIP(hipMemcpy(fc->d_cols, cols.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    }
    LSQ_HIP(hipMemcpy(fc->d_off, off.data(), ((size_t)n + 1) * sizeof(int), hipMemcpyHostToDevice));
    // a second call replaces the first (launches that read the old tables may still be in the stream)
    LSQ_HIP(hipStreamSynchronize(c->stream));
    lsq_fd_colouring_free(J);
    J->fdc = fc;
    guard.p = nullptr;
    if (h_ncolours) *h_ncolours = nc;
    return LSQ_OK;
}

// the values of a coloured CSC handle <- central differences of f at x
int fd_values_sparse(lsq_mat *J, const double *x, lsq_f_callback f, void *user) {
    lsq_ctx *c = J->ctx;
    const LsqFdColouring *fc = J->fdc;
    const int m = J->m, n = J->n;
    LSQ_TRY(lsq_ensure_csc(J));
    if (m <= 0 || n <= 0) return LSQ_OK;
    const size_t n2 = ((size_t)n + 1) & ~(size_t)1, m2 = ((size_t)m + 1) & ~(size_t)1;
    if (!J->d_fd) LSQ_HIP(hipMalloc(&J->d_fd, (2 * n2 + 2 * m2) * sizeof(double)));
    double *xp = J->d_fd, *xm = xp + n2, *fp = xm + n2, *fm = fp + m2;
    const int cap = c->num_cus * 8;
    LSQ_LAUNCH(k_fd_sparse_begin, dim3(std::max(1, std::min(lsq_div_up(n, LSQ_NT), cap))), dim3(LSQ_NT), 0, c->stream, n,
               (const int *)fc->d_colour, x, xp, xm);
    LSQ_HIP(hipGetLastError());
    for (int col = 0; col < fc->ncolours; ++col) {
        if (f(fp, xp, user) != 0 || f(fm, xm, user) != 0) {
            lsq_set_error("user callback reported failure");
            return LSQ_ECALLBACK;
        }
        const int b0 = fc->bound[col], b1 = fc->bound[col + 1], b2 = col + 1 < fc->ncolours ? fc->bound[col + 2] : b1;
        const int e0 = fc->ebound[col], e1 = fc->ebound[col + 1];
        const int work = std::max(e1 - e0, std::max(b1 - b0, b2 - b1));
        LSQ_LAUNCH(k_fd_sparse_step, dim3(std::max(1, std::min(lsq_div_up(work, LSQ_NT), cap))), dim3(LSQ_NT), 0, c->stream, b0,
                   b1, b2, e0, e1, (const int *)fc->d_cols, (const int *)fc->d_off, (const int *)J->csc.d_ptr,
                   (const int *)J->csc.d_idx, x, xp, xm, (const double *)fp, (const double *)fm, J->csc.d_val);
        LSQ_HIP(hipGetLastError());
    }
    return LSQ_OK;
}

}  // namespace

// which handles have a colouring here; LSQ_EARG with the reason otherwise
int lsq_fd_check(const lsq_mat *J, const char *who) {
    if (J->kind == LSQ_MAT_OP) {
        lsq_set_error("%s: central differences need a Jacobian with stored values; a matrix-free operator has none (give g!)", who);
        return LSQ_EARG;
    }
    if (J->d_cs_user) {
        lsq_set_error("%s: central differences write the stored values; on a column-scaled handle (lsq_mat_set_colscale) those are "
                      "V, not the Jacobian (remove the scale, or give g!)", who);
        return LSQ_EARG;
    }
    if (J->kind == LSQ_MAT_CSC && J->bd_blocks < 1 && J->br_blocks < 1 && !J->fdc) {
        lsq_set_error("%s: central differences on a general sparse pattern need a column colouring, and this handle has none "
                      "(types.jl:57: autodiff Jacobians are dense only). Attach one with lsq_mat_set_fd_colouring, or give g!",
                      who);
        return LSQ_EARG;
    }
    return LSQ_OK;
}

// the values of J <- central differences of f at x; the caller brings the other layouts of the handle up to date
// (lsq_mat_refresh, or lsq_ensure_csr behind lsq_call_g)
int lsq_fd_values(lsq_mat *J, const double *x, lsq_f_callback f, void *user) {
    if (J->fdc) return fd_values_sparse(J, x, f, user);
    lsq_ctx *c = J->ctx;
    FdShape s;
    if (J->kind == LSQ_MAT_DENSE) s = FdShape{1, J->m, 0, J->n, J->m};
    else if (J->bd_blocks > 0) s = FdShape{J->bd_blocks, J->bd_mb, J->bd_nb, 0, J->m};
    else s = FdShape{J->br_blocks, J->br_mb, J->br_nb, J->br_ng, J->m};
    const int m = J->m, n = J->n, colours = s.nb + s.ng;
    double *vals = J->kind == LSQ_MAT_DENSE ? J->d_dense : J->csc.d_val;
    LSQ_TRY(lsq_ensure_csc(J));       // (a device g! may have left the CSC-ordered copy behind its mirrors: it is the authority again)
    if (m <= 0 || n <= 0) return LSQ_OK;
    // x+ | x- | f+ | f-, each on a 16-byte boundary
    const size_t n2 = ((size_t)n + 1) & ~(size_t)1, m2 = ((size_t)m + 1) & ~(size_t)1;
    if (!J->d_fd) LSQ_HIP(hipMalloc(&J->d_fd, (2 * n2 + 2 * m2) * sizeof(double)));
    double *xp = J->d_fd, *xm = xp + n2, *fp = xm + n2, *fm = fp + m2;
    LSQ_LAUNCH(k_fd_begin, dim3(std::max(1, std::min(lsq_div_up(n, LSQ_NT), c->num_cus * 8))), dim3(LSQ_NT), 0, c->stream, s, n, x,
               xp, xm);
    LSQ_HIP(hipGetLastError());
    const bool v2 = (s.mb & 1) == 0 && fd_aligned16(fp) && fd_aligned16(fm) && fd_aligned16(vals);
    const int grid = std::max(1, std::min(lsq_div_up(v2 ? m / 2 : m, LSQ_NT), c->num_cus * 8));
    for (int col = 0; col < colours; ++col) {
        if (f(fp, xp, user) != 0 || f(fm, xm, user) != 0) {
            lsq_set_error("user callback reported failure");
            return LSQ_ECALLBACK;
        }
        const int next = col + 1 < colours ? col + 1 : -1;
        if (v2) LSQ_LAUNCH(k_fd_step<true>, dim3(grid), dim3(LSQ_NT), 0, c->stream, s, col, next, x, xp, xm, (const double *)fp,
                           (const double *)fm, vals);
        else LSQ_LAUNCH(k_fd_step<false>, dim3(grid), dim3(LSQ_NT), 0, c->stream, s, col, next, x, xp, xm, (const double *)fp,
                        (const double *)fm, vals);
        LSQ_HIP(hipGetLastError());
    }
    return LSQ_OK;
}

// g == NULL in lsq_optimize / lsq_optimize_batched: the loops run on these two callbacks with an LsqFdCall as their user
int lsq_fd_f_thunk(double *d_out, const double *d_x, void *user) {
    LsqFdCall *fc = (LsqFdCall *)user;
    return fc->f(d_out, d_x, fc->user);
}
int lsq_fd_g_thunk(lsq_mat *J, const double *d_x, void *user) {
    LsqFdCall *fc = (LsqFdCall *)user;
    fc->status = lsq_fd_values(J, d_x, fc->f, fc->user);
    return fc->status == LSQ_OK ? 0 : 1;
}

extern "C" int lsq_fd_jacobian(lsq_ctx *c, lsq_mat *J, const double *d_x, lsq_f_callback f, void *user) {
    LSQ_RANGE("lsq_fd_jacobian");
    if (!c || !J || !d_x || !f) {
        lsq_set_error("lsq_fd_jacobian: null argument");
        return LSQ_EARG;
    }
    if (J->ctx != c) {
        lsq_set_error("lsq_fd_jacobian: the Jacobian belongs to another context");
        return LSQ_EARG;
    }
    LSQ_TRY(lsq_fd_check(J, "lsq_fd_jacobian"));
    LSQ_HIP(hipSetDevice(c->device));
    const int st = lsq_fd_values(J, d_x, f, user);
    if (st != LSQ_OK) {
        // (some columns are new, some are not: the layouts of the handle at least agree with each other)
        char keep[512];
        snprintf(keep, sizeof(keep), "%s", lsq_last_error());
        (void)lsq_mat_refresh(J);
        lsq_set_error("%s", keep);
        return st;
    }
    return lsq_mat_refresh(J);
}

void lsq_fd_colouring_free(lsq_mat *J) {
    LsqFdColouring *fc = J->fdc;
    if (!fc) return;
    hipFree(fc->d_colour);
    hipFree(fc->d_cols);
    hipFree(fc->d_off);
    delete fc;
    J->fdc = nullptr;
}

extern "C" int lsq_csc_greedy_colouring(int m, int n, const int *h_colptr, const int *h_rowval, int *h_colour, int *h_ncolours) {
    LSQ_TRY(fd_check_pattern("lsq_csc_greedy_colouring", m, n, h_colptr, h_rowval));
    if (!h_ncolours || (n > 0 && !h_colour)) {
        lsq_set_error("lsq_csc_greedy_colouring: bad arguments");
        return LSQ_EARG;
    }
    try {
        *h_ncolours = fd_greedy(m, n, h_colptr, h_rowval, h_colour);
    } catch (const std::bad_alloc &) {
        lsq_set_error("lsq_csc_greedy_colouring: out of host memory on a %d x %d pattern", m, n);
        return LSQ_EHIP;
    }
    return LSQ_OK;
}

extern "C" int lsq_mat_set_fd_colouring(lsq_mat *J, const int *h_colour_or_null, int *h_ncolours) {
    if (!J) {
        lsq_set_error("lsq_mat_set_fd_colouring: null argument");
        return LSQ_EARG;
    }
    if (J->kind == LSQ_MAT_OP) {
        lsq_set_error("lsq_mat_set_fd_colouring: a matrix-free operator has no stored values to difference into");
        return LSQ_EARG;
    }
    if (J->kind == LSQ_MAT_DENSE || J->bd_blocks > 0 || J->br_blocks > 0) {
        lsq_set_error("lsq_mat_set_fd_colouring: a %s handle has its built-in colouring; only a plain CSC handle "
                      "(lsq_csc_create) takes one",
                      J->kind == LSQ_MAT_DENSE ? "dense" : J->bd_blocks > 0 ? "block-diagonal" : "bordered block-diagonal");
        return LSQ_EARG;
    }
    try {
        return fd_set_colouring_impl(J, h_colour_or_null, h_ncolours);
    } catch (const std::bad_alloc &) {
        lsq_set_error("lsq_mat_set_fd_colouring: out of host memory on a %d x %d pattern", J->m, J->n);
        return LSQ_EHIP;
    }
}

extern "C" int lsq_mat_fd_colouring(const lsq_mat *J, int *h_colour, int *h_ncolours) {
    if (!J || !h_ncolours) {
        lsq_set_error("lsq_mat_fd_colouring: null argument");
        return LSQ_EARG;
    }
    *h_ncolours = J->fdc ? J->fdc->ncolours : 0;
    if (J->fdc && h_colour) std::copy(J->fdc->colour.begin(), J->fdc->colour.end(), h_colour);
    return LSQ_OK;
}
