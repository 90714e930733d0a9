// Parameter covariance of a general sparse (CSC) Jacobian: lsq_sparse_gram (G = J'J, dense, from the sparse handle) and
// lsq_sparse_covariance, Cov = s^2 inv(J'J), s^2 = sum(f.^2) / (m - n) (or 1).
//
// Everything behind the Gram matrix is the dense covariance's (lsq_cov_dense.hip): the blocked Cholesky on a ready G
// (lsq_cholesky_blocked_factor, lsq_dense_mfma.hip; the one-workgroup kernel for the few small operands the dense path keeps
// away from it: lsq_cholesky_small_factor_ready, lsq_dense.hip), X = inv(U) (lsq_tri_inv_enqueue), k_cov_xxt and k_cov_stderr.
// They run on an inner dense LSQ_CHOLESKY lsq_solver that the LSMR() solver of the fit creates on first use (lsq_solver::inner).
//
// k_sp_gram: the upper triangle of G = J'J, column-major with leading dimension n, J never densified.
//   One wavefront owns one output column j and a dense accumulator acc[0 .. n) of its own in LDS (zero between columns).  It
//   walks the stored entries (i, v) of column j in CSC order, 64 at a time (row index, value and the row's two CSR pointers:
//   one load each per lane), and for every entry the row i of the CSR mirror up to column j (rows are sorted by column):
//   acc[c] += v * w for every (c, w) of the row.  The value of CSR position q is csc.d_val[d_map[q]] -- csr.d_val does not
//   exist on the sliced layouts; csr.d_ptr, csr.d_idx and d_map always do.
//   Sixteen rows are in flight at a time: the wavefront is cut into four 16-lane groups, group `sub` serves rows 4u + sub,
//   u = 0 .. 3, of the sixteen, with lanes across the row's entries; the index / map loads of all sixteen are issued, then the
//   value loads, then the LDS adds are APPLIED ONE ROW AFTER THE OTHER (u outer, sub inner: ascending row order) under the
//   group's exec mask.  A batch of sixteen in which some row has more than 16 entries takes the full-width form instead: one
//   row at a time, 64 lanes across it, looping, leaving the row at the first chunk that reaches past column j.
//   So every acc[c] receives its terms from one wavefront, in the order of the column's stored entries: no floating-point
//   atomics, nothing shared between columns, and the bits of column j do not depend on which wavefront takes it, on the grid,
//   or on the run.  Lanes of one row hit distinct c; a pattern with a repeated (row, column) pair -- the products sum such
//   pairs -- is noticed (equal neighbours in the sorted row) and that chunk is applied lane by lane.
//   At the end the wavefront stores acc[0 .. j] to G[j n + 0 .. j] (coalesced) and zeroes what it read.  Fused column-scaled
//   handle (d_colscale: the stored values are V, J = V diag(s)): G_kj = (acc_k s_k) s_j at that store, the S G_V S of the block
//   solvers.  Damping, where given, is added to the diagonal entry after everything else, as k_syrk_reduce adds it.  The strict
//   lower triangle is not written; the factorisations never read it.
//   Work per column grows with j (rows are cut at column j), so the columns are dealt out from the last one backwards, round
//   robin over all wavefronts of the grid, neighbouring columns to different workgroups: a static order, no ticket.
//   A workgroup holds W = min(4, floor(160 KiB / 8 n)) wavefronts: 4 up to n = 5120, 3 up to 6826, 2 up to 10240, then 1 up to
//   SG_MAX_N = 16384 (128 KiB); beyond that the entry refuses (windowed passes over the output rows are not built).
#include <algorithm>
#include <climits>
#include <cmath>

#include "lsq_solver.h"

int lsq_cholesky_blocked_factor(lsq_solver *s, int n, double *d_x, bool allow_tiles);   // lsq_dense_mfma.hip
int lsq_cholesky_small_factor_ready(lsq_solver *s, int n);                              // lsq_dense.hip
// lsq_cov_dense.hip: k_cov_xxt<false> and k_cov_stderr<false> on X = inv(U), whichever outputs are given
int lsq_cov_xxt_stderr(lsq_ctx *c, const double *X, int n, double s2, double *d_cov, double *d_stderr);

constexpr int SG_MAX_N = 16384;                       // columns: the accumulator of one wavefront must fit one workgroup's LDS
constexpr size_t SG_LDS_BUDGET = 160 * 1024;          // bytes of LDS one workgroup may hold on gfx950
constexpr int SG_MAX_WAVES = 4;

static inline int sg_waves(int n) {
    return (int)std::max<size_t>(1, std::min<size_t>(SG_MAX_WAVES, SG_LDS_BUDGET / (sizeof(double) * (size_t)n)));
}

// orders the LDS traffic of the wavefront's lanes in program order, for the compiler too (no instruction of its own: one
// wavefront's LDS operations complete in issue order)
__device__ __forceinline__ void sg_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ void __launch_bounds__(SG_MAX_WAVES * 64)
k_sp_gram(int n, const int *__restrict__ cp, const int *__restrict__ ri, const double *__restrict__ val,
          const int *__restrict__ rp, const int *__restrict__ ci, const int *__restrict__ map,
          const double *__restrict__ cs, const double *__restrict__ damp, double *__restrict__ G, int *__restrict__ info) {
    extern __shared__ __attribute__((aligned(16))) double sg_lds[];
    if (info && blockIdx.x == 0 && threadIdx.x == 0) *info = 0;   // the factorisation's status word, as k_syrk_reduce clears it
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nwv = blockDim.x >> 6;
    const int sub = lane >> 4, l16 = lane & 15;
    double *acc = sg_lds + (size_t)wv * n;
    for (int k = lane; k < n; k += 64) acc[k] = 0.0;
    sg_wave_sync();
    const int stride = nwv * gridDim.x;
    for (int j = n - 1 - (wv * (int)gridDim.x + (int)blockIdx.x); j >= 0; j -= stride) {
        const int e0 = cp[j], e1 = cp[j + 1];
        for (int base = e0; base < e1; base += 64) {
            const int e = base + lane;
            int rs = 0, re = 0;
            double v = 0.0;
            if (e < e1) {
                const int i = ri[e];
                v = val[e];
                rs = rp[i];
                re = rp[i + 1];
            }
            const int cnt = min(64, e1 - base);
            for (int g = 0; g < cnt; g += 16) {
                const bool is_long = lane >= g && lane < g + 16 && re - rs > 16;
                if (__ballot(is_long) == 0ull) {
                    // sixteen short rows: group `sub` serves rows g + 4 u + sub (lanes past cnt hold empty rows)
                    int c[4], mp[4];
                    double w[4], vv[4];
                    bool dup = false;
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int r = g + 4 * u + sub;
                        const int q = __shfl(rs, r) + l16;
                        const bool in = q < __shfl(re, r);
                        vv[u] = __shfl(v, r);
                        c[u] = in ? ci[q] : INT_MAX;
                        mp[u] = in ? map[q] : 0;
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        w[u] = c[u] <= j ? val[mp[u]] : 0.0;
                        const int prev = __shfl_up(c[u], 1);
                        dup = dup || (l16 > 0 && c[u] <= j && prev == c[u]);
                    }
                    if (__ballot(dup) == 0ull) {
#pragma unroll
                        for (int u = 0; u < 4; ++u)
#pragma unroll
                            for (int sg = 0; sg < 4; ++sg) {
                                if (sub == sg && c[u] <= j) acc[c[u]] += vv[u] * w[u];
                                sg_wave_sync();
                            }
                    } else {
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            for (int t = 0; t < 64; ++t) {      // (lane t: group t >> 4, entry t & 15 -- rows ascending, then entries)
                                if (lane == t && c[u] <= j) acc[c[u]] += vv[u] * w[u];
                                sg_wave_sync();
                            }
                    }
                } else {
                    const int rend = min(g + 16, cnt);
                    for (int r = g; r < rend; ++r) {
                        const int srs = __shfl(rs, r), sre = __shfl(re, r);
                        const double vr = __shfl(v, r);
                        for (int q0 = srs; q0 < sre; q0 += 64) {
                            const int q = q0 + lane;
                            const int c1 = q < sre ? ci[q] : INT_MAX;
                            const bool in = c1 <= j;
                            const double w1 = in ? val[map[q]] : 0.0;
                            const int prev = __shfl_up(c1, 1);
                            const bool dup = lane > 0 && in && prev == c1;
                            if (__ballot(dup) == 0ull) {
                                if (in) acc[c1] += vr * w1;
                                sg_wave_sync();
                            } else {
                                for (int t = 0; t < 64; ++t) {
                                    if (lane == t && in) acc[c1] += vr * w1;
                                    sg_wave_sync();
                                }
                            }
                            if (__ballot(in) != ~0ull) break;     // the row has reached past column j (or its end)
                        }
                    }
                }
            }
        }
        sg_wave_sync();
        const double sj = cs ? cs[j] : 1.0;
        double *Gj = G + (size_t)j * n;
        for (int k = lane; k <= j; k += 64) {
            double a = acc[k];
            acc[k] = 0.0;
            if (cs) a = (a * cs[k]) * sj;
            if (k == j && damp) a += damp[j];
            Gj[k] = a;
        }
        sg_wave_sync();
    }
}

// G = J'J (+ diag damp) of the CSC handle into the upper triangle of d_G, enqueued; info: nullptr or a status word to clear
static int sg_enqueue(lsq_mat *J, const double *d_damp, double *d_G, int *d_info) {
    lsq_ctx *c = J->ctx;
    const int n = J->n;
    LSQ_TRY(lsq_ensure_csc(J));      // the CSC-ordered values are what d_map addresses
    const int W = sg_waves(n);
    const size_t lds = (size_t)W * n * sizeof(double);
    // workgroups per CU that the LDS admits (small n), and no more wavefronts than columns
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(4, SG_LDS_BUDGET / lds));
    const int grid = std::max(1, std::min(lsq_div_up(n, W), c->num_cus * per_cu));
    LSQ_TRY(lsq_set_lds(c, (const void *)k_sp_gram, SG_LDS_BUDGET));
    LSQ_LAUNCH(k_sp_gram, dim3(grid), dim3(W * 64), lds, c->stream, n, (const int *)J->csc.d_ptr, (const int *)J->csc.d_idx,
               (const double *)J->csc.d_val, (const int *)J->csr.d_ptr, (const int *)J->csr.d_idx, (const int *)J->d_map,
               J->d_colscale, d_damp, d_G, d_info);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

static int sg_check_handle(const char *who, const lsq_mat *J, const char *dense_entry) {
    if (J->kind == LSQ_MAT_DENSE) {
        lsq_set_error("%s: the Jacobian is a dense handle (lsq_dense_create): %s", who, dense_entry);
        return LSQ_EARG;
    }
    if (J->kind != LSQ_MAT_CSC) {
        lsq_set_error("%s: the Jacobian is an operator handle (lsq_op_create), which stores no entries: J'J of an operator is n "
                      "pairs of lsq_mul, J'(J e_j)", who);
        return LSQ_EARG;
    }
    if (J->n > SG_MAX_N) {
        lsq_set_error("%s: n = %d is above the limit of %d columns (one wavefront's dense accumulator column, 8 n bytes, must fit "
                      "the 160 KiB of LDS of one workgroup); block-diagonal and bordered handles of any n have "
                      "lsq_solver_covariance", who, J->n, SG_MAX_N);
        return LSQ_EARG;
    }
    return LSQ_OK;
}

extern "C" int lsq_sparse_gram(lsq_mat *J, const double *d_damp, double *d_G) {
    LSQ_RANGE("lsq_sparse_gram");
    if (!J || !d_G) { lsq_set_error("lsq_sparse_gram: null argument"); return LSQ_EARG; }
    LSQ_TRY(sg_check_handle("lsq_sparse_gram", J, "J'J of a dense Jacobian is formed inside lsq_ldiv_damped / lsq_dense_covariance"));
    if (J->n <= 0) return LSQ_OK;
    LSQ_HIP(hipSetDevice(J->ctx->device));
    return sg_enqueue(J, d_damp, d_G, nullptr);
}

// G = J'J = U'U into in->d_chol and X = inv(U) into in->tri_X, enqueued; the factorisation's verdict in in->d_info[0]
static int sg_factor_and_invert(lsq_solver *in, lsq_mat *J, bool allow_tiles) {
    const int m = J->m, n = J->n;
    LSQ_TRY(sg_enqueue(J, nullptr, in->d_chol, in->d_info));
    if (lsq_cholesky_takes_blocked(m, n)) {
        LSQ_TRY(lsq_cholesky_blocked_factor(in, n, nullptr, allow_tiles));
        in->last_chol_path = in->last_chol_tiles ? 4 : 2;
    } else {
        LSQ_TRY(lsq_cholesky_small_factor_ready(in, n));
        in->last_chol_path = 1;
    }
    return lsq_tri_inv_enqueue(in, in->d_chol, n);
}

extern "C" int lsq_sparse_covariance(lsq_solver *s, lsq_mat *J, const double *d_f, double *d_cov, double *d_stderr,
                                     int *h_info) {
    LSQ_RANGE("lsq_sparse_covariance");
    if (!s || !J) { lsq_set_error("lsq_sparse_covariance: null argument"); return LSQ_EARG; }
    if (!d_cov && !d_stderr) {
        lsq_set_error("lsq_sparse_covariance: d_cov and d_stderr are both NULL: nothing to compute");
        return LSQ_EARG;
    }
    LSQ_TRY(sg_check_handle("lsq_sparse_covariance", J, "a Cholesky() solver on it has lsq_dense_covariance, a QR() solver "
                                                         "lsq_dense_qr_covariance"));
    if (s->kind != LSQ_LSMR) {
        lsq_set_error("lsq_sparse_covariance: needs the LSMR() solver created on this CSC Jacobian, the one a sparse fit owns; this "
                      "solver's kind is %d (a Cholesky() solver on a block-diagonal or bordered handle has lsq_solver_covariance)",
                      s->kind);
        return LSQ_EARG;
    }
    if (J->m != s->m || J->n != s->n) {
        lsq_set_error("lsq_sparse_covariance: this solver was allocated for a %d x %d Jacobian, got %d x %d; create the LSMR() "
                      "solver on the handle itself", s->m, s->n, J->m, J->n);
        return LSQ_EARG;
    }
    if (s->row_cb) {
        lsq_set_error("lsq_sparse_covariance: this solver has a row all-reduce hook (lsq_solver_set_row_allreduce): J is one rank's "
                      "row block and J'J would be that block's alone; switch the hook off, or sum lsq_sparse_gram over the ranks");
        return LSQ_EARG;
    }
    const int m = J->m, n = J->n;
    if (d_f && m <= n) {
        lsq_set_error("lsq_sparse_covariance: the residual variance sum(f.^2) / (m - n) needs m > n (got m = %d, n = %d); "
                      "pass d_f = NULL for the unscaled inv(J'J)", m, n);
        return LSQ_EARG;
    }
    if (h_info) h_info[0] = 0;
    if (n <= 0) return LSQ_OK;
    lsq_ctx *c = s->ctx;
    LSQ_HIP(hipSetDevice(c->device));
    if (!s->inner) {            // the dense Cholesky() solver behind the Gram matrix: n^2 doubles, more on first use
        lsq_solver *in = new lsq_solver();
        in->ctx = c;
        in->kind = LSQ_CHOLESKY;
        in->for_lm = 1;
        in->m = m;
        in->n = n;
        const int st = lsq_dense_solver_alloc(in);
        if (st != LSQ_OK) {
            lsq_dense_solver_free(in);
            delete in;
            return st;
        }
        s->inner = in;
    }
    lsq_solver *in = s->inner;
    double ssq = 0.0;
    int st4[4] = {0, 0, 0, 0};
    for (int attempt = 0; attempt < 2; ++attempt) {
        // (the factorisation overwrites d_chol: the Gram kernel runs again for the retry)
        LSQ_TRY(sg_factor_and_invert(in, J, attempt == 0));
        // the one wait of the call: the variance (on the first round) and the factorisation's verdict behind it
        if (d_f && attempt == 0) LSQ_TRY(lsq_sumsq(c, m, d_f, &ssq));
        LSQ_TRY(lsq_read_ints(c, in->d_info, nullptr, nullptr, nullptr, st4));
        if (st4[0] != -1 || in->fb_tiles.off()) break;
        in->fb_tiles.gave_up(c, LSQ_FB_CHOL_TILES);    // the one-launch factorisation gave up on a wait: panel launches, once more
    }
    in->fb_tiles.solve_done(in->last_chol_path == 4);
    const int info = st4[0];
    if (info != 0) {
        if (h_info) h_info[0] = info;
        lsq_set_error("PosDefException: matrix is not positive definite; Cholesky failed at %d", info);
        return LSQ_ENOTPD;
    }
    const double s2 = d_f ? ssq / (double)(m - n) : 1.0;
    return lsq_cov_xxt_stderr(c, in->tri_X, n, s2, d_cov, d_stderr);
}
