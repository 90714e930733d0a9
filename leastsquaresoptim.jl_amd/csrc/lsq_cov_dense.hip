// Parameter covariance of a plain dense Jacobian: lsq_dense_covariance, Cov = s^2 inv(J'J), s^2 = sum(f.^2) / (m - n) (or 1).
//
// Everything up to the last product exists elsewhere and is only enqueued here:
//   1. G = J'J and G = U'U: lsq_cholesky_blocked (lsq_dense_mfma.hip: MFMA SYRK, one-launch or panel factorisation), or -- on
//      the operands lsq_cholesky_solve keeps away from the blocked path -- lsq_cholesky_small_factor (lsq_dense.hip)
//   2. X = inv(U) into the upper triangle of s->tri_X: lsq_tri_inv_enqueue (lsq_qr.hip: k_tri_diaginv + k_tri_level)
//   3. k_cov_xxt: inv(G) = X X', one workgroup per 64 x 64 upper tile (I, J), I <= J:  C_IJ = sum_{K >= J} X_IK X_JK'.
//      Only K >= J contributes (X_JK = 0 for K < J); the diagonal blocks of X are masked below their diagonal on the way into
//      LDS -- tri_X is never written there, and what it holds may be NaN -- and rows, columns and k's past n likewise.  The K
//      blocks are added in index order into one set of accumulators: no split over K, no floating-point atomics, the same
//      bits on every run.  Accumulators times s^2 go to (i, j) and to the mirror (j, i); in a diagonal tile only i <= j is
//      stored.  Tile column J has nt - J blocks of work, so the tiles are numbered by columns: the long ones start first.
//   4. k_cov_stderr: s sqrt(sum_{k >= i} X_ik^2), one wavefront per row in a fixed lane-strided order and a fixed butterfly;
//      a kernel of its own, so that its bits do not depend on whether the covariance was asked for.  It agrees with
//      sqrt(diag(cov)) to rounding only (the MFMA unit adds the same squares in another order).
// lsq_dense_qr_covariance (at the end of the file) feeds the same two kernels, or their un-permuting variants, with X = inv(R)
// of the QR() factor.
#include <algorithm>
#include <cmath>

#include "lsq_solver.h"

int lsq_cholesky_blocked(lsq_solver *s, lsq_mat *J, const double *d_damp, double *d_x, double *d_dmax, bool allow_tiles,
                         const double *d_y);   // lsq_dense_mfma.hip

constexpr int CX_T = 64;            // tile
constexpr int CX_KC = 32;           // k's staged per step
constexpr int CX_KS = CX_KC + 2;    // LDS row stride (doubles)
typedef double cx_v4d __attribute__((ext_vector_type(4)));

// wave and fragment layout of k_tri_level (lsq_qr.hip): four wavefronts own the 32 x 32 quadrants, 2 x 2 MFMA 16 x 16 x 4 tiles
// each; operand A: lane & 15 = row, lane >> 4 = k; operand B: lane & 15 = column; accumulator r: row (lane >> 4) + 4 r
// PERM: accumulator (a, b) of X X' goes to (jp[a], jp[b]) and to its mirror (lsq_dense_qr_covariance on a pivoted factor, J P = Q R)
template <bool PERM>
__global__ void __launch_bounds__(256)
k_cov_xxt(const double *__restrict__ X, int n, double s2, double *__restrict__ C, const int *__restrict__ jp) {
    __shared__ double sA[CX_T * CX_KS];
    __shared__ double sB[CX_T * CX_KS];
    int t = blockIdx.x, tj = 0;
    while (t > tj) { t -= tj + 1; ++tj; }      // tile column tj holds tiles ti = 0 .. tj
    const int ti = t;
    const int i0 = ti * CX_T, j0 = tj * CX_T;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wr = (w >> 1) * 32, wc = (w & 1) * 32;
    cx_v4d acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = (cx_v4d){0.0, 0.0, 0.0, 0.0};
    // staging: lane = row of X (coalesced down a column k), 8 k's per thread; A(m, k) = X(i0 + m, k), B(k, c) = X(j0 + c, k)
    const int am = tid & 63, akq = (tid >> 6) * 8;
    const int ia = i0 + am, jb = j0 + am;
    const bool rows_full = j0 + CX_T <= n;      // (then i0 + 64 <= n as well)
    double ra[8], rb[8];
    auto fetch = [&](int k0) {
        if (rows_full && k0 >= j0 + CX_T && k0 + CX_KC <= n) {   // past both diagonal blocks, inside the matrix: full blocks
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const size_t col = (size_t)(k0 + akq + q) * n;
                ra[q] = X[col + ia];
                rb[q] = X[col + jb];
            }
        } else {                                // X(r, k) exists for r <= k < n only
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int k = k0 + akq + q;
                ra[q] = (k < n && ia <= k) ? X[(size_t)k * n + ia] : 0.0;
                rb[q] = (k < n && jb <= k) ? X[(size_t)k * n + jb] : 0.0;
            }
        }
    };
    fetch(j0);
    for (int k0 = j0; k0 < n; k0 += CX_KC) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            sA[am * CX_KS + akq + q] = ra[q];
            sB[am * CX_KS + akq + q] = rb[q];
        }
        __syncthreads();
        if (k0 + CX_KC < n) fetch(k0 + CX_KC);
#pragma unroll
        for (int kk = 0; kk < CX_KC; kk += 4) {
            const int ko = kk + (lane >> 4);
            const double a0 = sA[(wr + (lane & 15)) * CX_KS + ko];
            const double a1 = sA[(wr + 16 + (lane & 15)) * CX_KS + ko];
            const double b0 = sB[(wc + (lane & 15)) * CX_KS + ko];
            const double b1 = sB[(wc + 16 + (lane & 15)) * CX_KS + ko];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = i0 + wr + a * 16 + (lane >> 4) + 4 * r;
                const int col = j0 + wc + b * 16 + (lane & 15);
                if (row < n && col < n && row <= col) {        // (row <= col: always true off the diagonal tiles)
                    const double v = s2 * acc[a][b][r];
                    if constexpr (PERM) {
                        const size_t pr = (size_t)jp[row], pc = (size_t)jp[col];
                        C[pc * n + pr] = v;
                        if (row != col) C[pr * n + pc] = v;
                    } else {
                        C[(size_t)col * n + row] = v;
                        if (row != col) C[(size_t)row * n + col] = v;
                    }
                }
            }
}

// PERM: row i of X is parameter jp[i]
template <bool PERM>
__global__ void __launch_bounds__(256)
k_cov_stderr(const double *__restrict__ X, int n, double s, double *__restrict__ se, const int *__restrict__ jp) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    double acc = 0.0;
    for (int k = i + lane; k < n; k += 64) {
        const double x = X[(size_t)k * n + i];
        acc += x * x;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) se[PERM ? jp[i] : i] = s * sqrt(acc);
}

// the n x n upper triangle of a factor that stands in a taller buffer (leading dimension ld > n, reflectors below the
// diagonal) into a leading-dimension-n image: what lsq_tri_inv_enqueue and k_cov_xxt read.  Below the diagonal U is left alone.
__global__ void __launch_bounds__(256)
k_cov_tri_gather(const double *__restrict__ R, int ld, int n, double *__restrict__ U) {
    const long long tot = (long long)n * n;
    for (long long e = blockIdx.x * 256LL + threadIdx.x; e < tot; e += (long long)gridDim.x * 256) {
        const int r = (int)(e % n), cidx = (int)(e / n);
        if (r <= cidx) U[e] = R[(size_t)cidx * ld + r];
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// G = J'J = U'U into s->d_chol and X = inv(U) into s->tri_X, enqueued; the factorisation's verdict in s->d_info[0]
static int factor_and_invert(lsq_solver *s, lsq_mat *J, bool allow_tiles) {
    const int m = J->m, n = J->n;
    if (lsq_cholesky_takes_blocked(m, n)) {
        LSQ_TRY(lsq_cholesky_blocked(s, J, nullptr, nullptr, nullptr, allow_tiles, nullptr));
        s->last_chol_path = s->last_chol_tiles ? 4 : 2;
    } else {
        LSQ_TRY(lsq_cholesky_small_factor(s, J));
        s->last_chol_path = 1;
    }
    return lsq_tri_inv_enqueue(s, s->d_chol, n);
}

// the last two launches on X = inv(U) in natural order: s2 X X' into d_cov, sqrt(s2) times the row norms of X into d_stderr,
// whichever is given (also lsq_sparse_covariance, lsq_cov_sparse.hip)
int lsq_cov_xxt_stderr(lsq_ctx *c, const double *X, int n, double s2, double *d_cov, double *d_stderr) {
    if (d_cov) {
        const int nt = lsq_div_up(n, CX_T);
        LSQ_LAUNCH(k_cov_xxt<false>, dim3(nt * (nt + 1) / 2), dim3(256), 0, c->stream, X, n, s2, d_cov, (const int *)nullptr);
    }
    if (d_stderr) LSQ_LAUNCH(k_cov_stderr<false>, dim3(lsq_div_up(n, 4)), dim3(256), 0, c->stream, X, n, sqrt(s2), d_stderr,
                                 (const int *)nullptr);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

extern "C" int lsq_dense_covariance(lsq_solver *s, lsq_mat *J, const double *d_f, double *d_cov, double *d_stderr,
                                    int *h_info) {
    LSQ_RANGE("lsq_dense_covariance");
    if (!s || !J) { lsq_set_error("lsq_dense_covariance: null argument"); return LSQ_EARG; }
    if (!d_cov && !d_stderr) {
        lsq_set_error("lsq_dense_covariance: d_cov and d_stderr are both NULL: nothing to compute");
        return LSQ_EARG;
    }
    if (s->kind != LSQ_CHOLESKY || s->bd_blocks != 0 || s->br_blocks != 0 || !s->d_chol) {
        lsq_set_error("lsq_dense_covariance: needs a Cholesky() solver created on a dense Jacobian (lsq_dense_create); this "
                      "solver's kind is %d%s", s->kind, (s->bd_blocks || s->br_blocks) ? ", on a block-diagonal handle" : "");
        return LSQ_EARG;
    }
    if (J->kind != LSQ_MAT_DENSE) {
        lsq_set_error("lsq_dense_covariance: the Jacobian is not a dense handle (lsq_dense_create); block-diagonal and bordered "
                      "handles have lsq_solver_covariance, CSC and operator handles are not offered");
        return LSQ_EARG;
    }
    if (J->m != s->m || J->n != s->n) {
        lsq_set_error("lsq_dense_covariance: this solver was allocated for a %d x %d Jacobian, got %d x %d", s->m, s->n, J->m, J->n);
        return LSQ_EARG;
    }
    const int m = J->m, n = J->n;
    if (d_f && m <= n) {
        lsq_set_error("lsq_dense_covariance: the residual variance sum(f.^2) / (m - n) needs m > n (got m = %d, n = %d); "
                      "pass d_f = NULL for the unscaled inv(J'J)", m, n);
        return LSQ_EARG;
    }
    if (h_info) h_info[0] = 0;
    if (n <= 0) return LSQ_OK;
    lsq_ctx *c = s->ctx;
    LSQ_HIP(hipSetDevice(c->device));
    double ssq = 0.0;
    int st4[4] = {0, 0, 0, 0};
    for (int attempt = 0; attempt < 2; ++attempt) {
        LSQ_TRY(factor_and_invert(s, J, attempt == 0));
        // the one wait of the call: the variance (on the first round) and the factorisation's verdict behind it
        if (d_f && attempt == 0) LSQ_TRY(lsq_sumsq(c, m, d_f, &ssq));
        LSQ_TRY(lsq_read_ints(c, s->d_info, nullptr, nullptr, nullptr, st4));
        if (st4[0] != -1 || s->fb_tiles.off()) break;
        s->fb_tiles.gave_up(c, LSQ_FB_CHOL_TILES);     // the one-launch factorisation gave up on a wait: panel launches, once more
    }
    s->fb_tiles.solve_done(s->last_chol_path == 4);
    const int info = st4[0];
    if (info != 0) {
        if (h_info) h_info[0] = info;
        lsq_set_error("PosDefException: matrix is not positive definite; Cholesky failed at %d", info);
        return LSQ_ENOTPD;
    }
    const double s2 = d_f ? ssq / (double)(m - n) : 1.0;
    return lsq_cov_xxt_stderr(c, s->tri_X, n, s2, d_cov, d_stderr);
}

// ---------------------------------------------------------------------------------------------
// lsq_dense_qr_covariance: the same from the QR() factor, J P = Q R: Cov = s^2 P X X' P', X = inv(R) -- J'J is never formed,
// so the condition number is not squared.  The factor is the one lsq_qr_solve enqueues for this operand, undamped, with a
// solver-owned zero right-hand side (a for_lm solver stacks n zero rows: the same R, and the same (M, n) workspace as its
// solves); its x is discarded.  Where that solve leaves things (lsq_solver::qr_R / qr_ldr / qr_X, pivots in d_tau, the rank in
// d_info[0]):
//   certified (qr_path 3): X = Qr2Work::Xinv already, jp = identity: k_cov_xxt / k_cov_stderr as above
//   pivoted sweep on the stage-1 triangle (2): R in pivoted order, leading dimension n: lsq_tri_inv_enqueue on it
//   one-stage (1): R at the top of s->d_qr, leading dimension M: k_cov_tri_gather into s->d_T, then lsq_tri_inv_enqueue
// and on the pivoted ones k_cov_xxt<true> / k_cov_stderr<true> un-permute on the way out.
// ---------------------------------------------------------------------------------------------
// The two halves of lsq_dense_qr_covariance around its wait (also lsq_bordered_qr_covariance, lsq_cov_bordered.hip, on the inner
// QR() of a BorderedQR() solver, which reads the rank beside its own verdict).  Everything in front of the wait, enqueued: the
// solve on zeros and, off the certified path, the inverse of the pivoted triangle; X = inv(R), jp = the pivots or nullptr
int lsq_dense_qr_cov_factor(lsq_solver *s, lsq_mat *J, const double **Xout, const int **jpout) {
    lsq_ctx *c = s->ctx;
    const int m = J->m, n = J->n;
    // zeros (the right-hand side, m; the damping of a for_lm solver, n <= m) | the solve's x, discarded (n)
    if (!s->d_cov_buf) {
        LSQ_HIP(hipMalloc(&s->d_cov_buf, ((size_t)m + n + 8) * sizeof(double)));
        LSQ_HIP(hipMemsetAsync(s->d_cov_buf, 0, (size_t)m * sizeof(double), c->stream));
    }
    const double *zero = s->d_cov_buf;
    LSQ_TRY(lsq_qr_solve(s, J, zero, s->for_lm ? zero : nullptr, s->d_cov_buf + m, nullptr));
    const double *X = s->qr_X;
    const int *jp = nullptr;
    if (s->last_qr_path != 3 || !X) {
        const double *U = s->qr_R;
        if (s->qr_ldr != n) {
            const long long tot = (long long)n * n;
            const int g = (int)std::min<long long>((tot + 255) / 256, (long long)c->num_cus * 8);
            LSQ_LAUNCH(k_cov_tri_gather, dim3(g), dim3(256), 0, c->stream, U, s->qr_ldr, n, s->d_T);
            U = s->d_T;
        }
        LSQ_TRY(lsq_tri_inv_enqueue(s, U, n));
        X = s->tri_X;
        jp = (const int *)s->d_tau;
    }
    *Xout = X;
    *jpout = jp;
    return LSQ_OK;
}

// ... and behind it, once the rank is known to be n: s2 P X X' P' into d_cov, the standard errors into d_stderr (either may be null)
int lsq_dense_qr_cov_finish(lsq_solver *s, int n, const double *X, const int *jp, double s2, double *d_cov, double *d_stderr) {
    lsq_ctx *c = s->ctx;
    const int nt = lsq_div_up(n, CX_T);
    if (jp) {
        if (d_cov) LSQ_LAUNCH(k_cov_xxt<true>, dim3(nt * (nt + 1) / 2), dim3(256), 0, c->stream, X, n, s2, d_cov, jp);
        if (d_stderr) LSQ_LAUNCH(k_cov_stderr<true>, dim3(lsq_div_up(n, 4)), dim3(256), 0, c->stream, X, n, sqrt(s2), d_stderr, jp);
    } else {
        if (d_cov) LSQ_LAUNCH(k_cov_xxt<false>, dim3(nt * (nt + 1) / 2), dim3(256), 0, c->stream, X, n, s2, d_cov, jp);
        if (d_stderr) LSQ_LAUNCH(k_cov_stderr<false>, dim3(lsq_div_up(n, 4)), dim3(256), 0, c->stream, X, n, sqrt(s2), d_stderr, jp);
    }
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

extern "C" int lsq_dense_qr_covariance(lsq_solver *s, lsq_mat *J, const double *d_f, double *d_cov, double *d_stderr,
                                       int *h_info) {
    LSQ_RANGE("lsq_dense_qr_covariance");
    if (!s || !J) { lsq_set_error("lsq_dense_qr_covariance: null argument"); return LSQ_EARG; }
    if (!d_cov && !d_stderr) {
        lsq_set_error("lsq_dense_qr_covariance: d_cov and d_stderr are both NULL: nothing to compute");
        return LSQ_EARG;
    }
    if (s->kind != LSQ_QR || !s->d_qr) {
        lsq_set_error("lsq_dense_qr_covariance: needs a QR() solver created on a dense Jacobian (lsq_dense_create); this "
                      "solver's kind is %d (a Cholesky() solver has lsq_dense_covariance)", s->kind);
        return LSQ_EARG;
    }
    if (J->kind != LSQ_MAT_DENSE) {
        lsq_set_error("lsq_dense_qr_covariance: the Jacobian is not a dense handle (lsq_dense_create)");
        return LSQ_EARG;
    }
    if (J->m != s->m || J->n != s->n) {
        lsq_set_error("lsq_dense_qr_covariance: this solver was allocated for a %d x %d Jacobian, got %d x %d", s->m, s->n, J->m, J->n);
        return LSQ_EARG;
    }
    const int m = J->m, n = J->n;
    if (m < n) {
        lsq_set_error("lsq_dense_qr_covariance: inv(J'J) needs m >= n (got m = %d, n = %d)", m, n);
        return LSQ_EARG;
    }
    if (d_f && m <= n) {
        lsq_set_error("lsq_dense_qr_covariance: the residual variance sum(f.^2) / (m - n) needs m > n (got m = %d, n = %d); "
                      "pass d_f = NULL for the unscaled inv(J'J)", m, n);
        return LSQ_EARG;
    }
    if (h_info) h_info[0] = 0;
    if (n <= 0) return LSQ_OK;
    lsq_ctx *c = s->ctx;
    LSQ_HIP(hipSetDevice(c->device));
    const double *X = nullptr;
    const int *jp = nullptr;
    LSQ_TRY(lsq_dense_qr_cov_factor(s, J, &X, &jp));
    // the one wait beyond the solve's own: the variance and, behind it, the rank decision of the solve
    double ssq = 0.0;
    int st4[4] = {0, 0, 0, 0};
    if (d_f) LSQ_TRY(lsq_sumsq(c, m, d_f, &ssq));
    LSQ_TRY(lsq_read_ints(c, s->d_info, nullptr, nullptr, nullptr, st4));
    const int rank = st4[0];
    s->last_rank = rank;
    if (h_info) h_info[0] = rank;
    if (rank < n) {
        lsq_set_error("RankDeficientException(%d): lsq_dense_qr_covariance: the Jacobian has rank %d < n = %d (xGELSY's decision at "
                      "rcond = n eps); a pseudo-inverse covariance is not offered", rank, rank, n);
        return LSQ_ERANK;
    }
    const double s2 = d_f ? ssq / (double)(m - n) : 1.0;
    return lsq_dense_qr_cov_finish(s, n, X, jp, s2, d_cov, d_stderr);
}
