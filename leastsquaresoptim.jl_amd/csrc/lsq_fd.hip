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
#include <algorithm>
#include <cstdint>

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

bool fd_aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

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
    if (J->kind == LSQ_MAT_CSC && J->bd_blocks < 1 && J->br_blocks < 1) {
        lsq_set_error("%s: central differences are available on dense, block-diagonal and bordered block-diagonal handles; a "
                      "general sparse pattern needs a column colouring, which is not built (types.jl:57: autodiff Jacobians "
                      "are dense only). Give g!", who);
        return LSQ_EARG;
    }
    return LSQ_OK;
}

// the values of J <- central differences of f at x; the caller brings the other layouts of the handle up to date
// (lsq_mat_refresh, or lsq_ensure_csr behind lsq_call_g)
int lsq_fd_values(lsq_mat *J, const double *x, lsq_f_callback f, void *user) {
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
