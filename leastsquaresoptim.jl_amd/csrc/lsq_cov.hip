// Parameter covariance of the many-small-fits handles: lsq_solver_covariance (the dispatch) and its block-diagonal half.
//
// J = blkdiag(J_1 .. J_B) (lsq_blockdiag_create, nb <= 64): Cov_b = s_b^2 inv(J_b'J_b), s_b^2 = sum(f_b.^2) / (mb - nb) (or 1),
// per block and in ONE pass over the values -- the cost of one solve.  k_bd_cov has the geometry and the streaming Gram loop
// of k_bd_solve (lsq_blockdiag.hip; restated here, so that k_bd_solve compiles to what it did): 16 < nb <= 64 one 256-thread
// workgroup per block (G = 4), nb <= 16 one wavefront per block, four per workgroup (G = 1).  With G_b in LDS (column scale
// applied, identity padding up to 16 NT, NT = ceil(nb / 16)):
//   1. G_b = U'U, the unpivoted blocked Cholesky of k_bd_solve<.., false>; s64_chol16 leaves inv(U_kk)' in W
//   2. Y = inv(U)' on NT tile rows (lsq_cov.h: the diagonal blocks are already there, NT - 1 levels of MFMA tile products
//      below them).  The LDS matrices keep k_bd_solve's size, 16 NT rows, instead of being padded to the 64 columns that
//      s64_chol_inverse is written for: two workgroups per CU still fit at nb = 64
//   3. Cov = Y'Y, upper 16 x 16 tiles on the fp64 MFMA unit
//   4. accumulators * s_b^2 straight to global memory, every entry also to its mirror position
// sum(f_b.^2) rides in the streaming loop (32 lanes, each its rows over the chunks, then a butterfly over those lanes): every
// sum has a fixed association, a block never reads another block's data, no floating-point atomics -- block b's bits do not
// depend on B, on the launch mode or on the run.  A block whose factorisation meets a non-positive pivot gets NaN everywhere
// and its column in binfo[b]; the other blocks do not notice.
// The bordered half (lsq_blockdiag_bordered_create) lives beside the solve it shares its elimination with: lsq_bordered.hip.
#include <cmath>

#include "lsq_solver.h"
#include "lsq_cov.h"

constexpr int CV_R = 32;           // rows per streamed chunk
constexpr int CV_CS = CV_R + 2;    // column stride of the staged chunk (doubles)
constexpr int CV_MISC = 8;         // doubles behind M and W: [0] sum(f_b.^2), [1] (as ints) first failing column

// doubles of LDS per block (= per group of G wavefronts)
static inline size_t cv_group_doubles(int nb) { return 2 * (size_t)(16 * ((nb + 15) / 16)) * S64_LS + CV_MISC; }

template <int G>
__global__ void __launch_bounds__(256)
k_bd_cov(int B, int mb, int nb, const double *__restrict__ vals, const double *__restrict__ scale,
         const double *__restrict__ f, double *__restrict__ cov, double *__restrict__ se, int *__restrict__ binfo) {
    extern __shared__ double cv_lds[];
    constexpr int GT = 64 * G;                 // threads per block of the matrix
    constexpr int TPW = G == 4 ? 3 : 1;        // upper tiles per wavefront (10 tiles over 4 wavefronts / 1 tile)
    constexpr int CP = GT / 32;                // columns per load pass
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wg = G == 4 ? __builtin_amdgcn_readfirstlane(wv) : 0;      // wavefront inside its group
    const int gt = G == 4 ? tid : lane;                                  // thread inside its group
    const int b = G == 4 ? (int)blockIdx.x : (int)blockIdx.x * 4 + wv;
    const bool live = b < B;
    const int NT = (nb + 15) >> 4, ncp = 16 * NT;
    const int msz = ncp * S64_LS;
    double *M = cv_lds + (G == 4 ? 0 : wv) * (size_t)(2 * msz + CV_MISC);
    double *W = M + msz;                       // chunk staging while streaming, then Y = inv(U)'
    double *ch = W;
    double *misc_d = W + msz;                  // [0] sum(f_b.^2)
    int *misc_i = (int *)(misc_d + 1);         // [0] first failing column
    const int ij = lane & 15, kq = lane >> 4;

    int ti[TPW], tj[TPW];
    bool has[TPW];
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
        const int t = wg + G * q;
        has[q] = t < NT * (NT + 1) / 2;
        int a = 0, r = t;
        while (has[q] && r >= NT - a) { r -= NT - a; ++a; }
        ti[q] = has[q] ? a : 0;
        tj[q] = has[q] ? a + r : 0;
    }

    // ---- stream J_b: G (upper tiles), sum(f_b.^2) ----
    const size_t vbase = live ? (size_t)b * mb * nb : 0;
    const size_t fbase = live ? (size_t)b * mb : 0;
    const int lr = gt & 31, c0 = gt >> 5;
    double reg[8], freg = 0.0, ssq = 0.0;
    auto load = [&](int row0) {
        const int row = row0 + lr;
        const bool ok = live && row < mb;
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int c = c0 + p * CP;
            reg[p] = (ok && c < nb) ? vals[vbase + (size_t)c * mb + row] : 0.0;
        }
        if (f && gt < 32) freg = ok ? f[fbase + row] : 0.0;
    };
    s64_v4d acc[TPW];
#pragma unroll
    for (int q = 0; q < TPW; ++q) acc[q] = s64_v4d{0.0, 0.0, 0.0, 0.0};
    const int nch = (mb + CV_R - 1) / CV_R;
    load(0);
    for (int c = 0; c < nch; ++c) {
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int col = c0 + p * CP;
            if (col < ncp) ch[col * CV_CS + lr] = reg[p];      // (columns nb .. ncp-1: zeros)
        }
        ssq += freg * freg;                                    // (lanes 32 .. of the group: zeros)
        __syncthreads();
        if (c + 1 < nch) load((c + 1) * CV_R);                 // in flight during the tile products
#pragma unroll
        for (int ks = 0; ks < CV_R / 4; ++ks) {
            const int kk = 4 * ks + kq;
#pragma unroll
            for (int q = 0; q < TPW; ++q) {
                if (has[q]) {
                    const double a = ch[(16 * ti[q] + ij) * CV_CS + kk];
                    const double bb = ch[(16 * tj[q] + ij) * CV_CS + kk];
                    acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bb, acc[q], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
    // ---- G (column-scaled handle: S G_V S) into M ----
    auto sc = [&](int k) { return (scale && live && k < nb) ? scale[(size_t)b * nb + k] : 1.0; };
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
        if (has[q]) {
            const int j = 16 * tj[q] + ij;
            const double sj = sc(j);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 16 * ti[q] + kq + 4 * r;
                M[i * S64_LS + j] = scale ? acc[q][r] * (sc(i) * sj) : acc[q][r];
            }
        }
    }
    if (wg == 0) {                             // sum(f_b.^2): lanes 0..31 hold the rows' sums, a fixed butterfly over them
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) ssq += __shfl_xor(ssq, off);
        if (lane == 0) { misc_d[0] = ssq; misc_i[0] = 0; }
    }
    __syncthreads();
    if (gt < ncp && (!live || gt >= nb)) M[gt * S64_LS + gt] = 1.0;    // padding: identity
    __syncthreads();

    // ---- G = U'U, unpivoted (the blocked scheme of k_bd_solve<.., false> on NT tile rows); W: inv(U_kk)' ----
    for (int kb = 0; kb < NT; ++kb) {
        const int o = 16 * kb;
        if (wg == 0) {
            const int bad = s64_chol16(M, W, o, lane);
            if (bad && lane == 0 && misc_i[0] == 0) misc_i[0] = o + bad;
        }
        __syncthreads();
        const int nt = NT - 1 - kb;
        for (int q = wg; q < nt; q += G) {             // row panel: U[o.., t] = inv(U_kk)' G[o.., t]
            const int t = kb + 1 + q;
            s64_v4d a = {0.0, 0.0, 0.0, 0.0};
            s64_tile_mma<false, false>(a, W, o, o, M, o, 16 * t, 1, lane);
            s64_tile_store<false>(M, o, 16 * t, a, 1.0, lane);
        }
        __syncthreads();
        for (int q = wg; q < nt * (nt + 1) / 2; q += G) {   // trailing tiles (ta <= tb) -= U[o.., ta]' U[o.., tb]
            int t = 0, r = q;
            while (r >= nt - t) { r -= nt - t; ++t; }
            const int ta = kb + 1 + t, tb = ta + r;
            s64_v4d a = {0.0, 0.0, 0.0, 0.0};
            s64_tile_mma<true, false>(a, M, o, 16 * ta, M, o, 16 * tb, 1, lane);
            s64_tile_store<true>(M, 16 * ta, 16 * tb, a, -1.0, lane);
        }
        __syncthreads();
    }
    const int fail = misc_i[0];
    // ---- Y = inv(U)', Cov = s^2 Y'Y ----
    cov_inv_levels<G>(M, W, NT, wg, lane);
    double s2 = f ? misc_d[0] / (double)(mb - nb) : 1.0;
    if (fail) s2 = NAN;                        // (NaN times whatever the failed factorisation left is NaN)
    if (!live) return;                         // (no barrier below)
    if (binfo && gt == 0) binfo[b] = fail;
    double *cb = cov ? cov + (size_t)b * nb * nb : nullptr;
    double *sb = se ? se + (size_t)b * nb : nullptr;
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
        if (has[q]) {
            const s64_v4d a = cov_tile(W, W, NT, ti[q], tj[q], lane);
            cov_store(cb, sb, nb, ti[q], tj[q], a, s2, lane);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
template <int G>
static int bd_cov_launch(lsq_ctx *c, lsq_mat *J, const double *d_f, double *d_cov, double *d_stderr, int *d_binfo) {
    const int B = J->bd_blocks;
    const size_t lds = (G == 4 ? 1 : 4) * cv_group_doubles(J->bd_nb) * sizeof(double);
    LSQ_TRY(lsq_set_lds(c, (const void *)k_bd_cov<G>, lds));
    const int grid = G == 4 ? B : (B + 3) / 4;
    LSQ_LAUNCH((k_bd_cov<G>), dim3(grid), dim3(256), lds, c->stream, B, J->bd_mb, J->bd_nb, (const double *)J->csc.d_val,
               J->d_colscale, d_f, d_cov, d_stderr, d_binfo);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

static int blockdiag_covariance(lsq_solver *s, lsq_mat *J, const double *d_f, double *d_cov, double *d_stderr, int *h_info) {
    lsq_ctx *c = s->ctx;
    if (J->kind != LSQ_MAT_CSC || J->bd_blocks != s->bd_blocks || J->bd_mb != s->bd_mb || J->bd_nb != s->bd_nb ||
        J->m != s->m || J->n != s->n) {
        lsq_set_error("lsq_solver_covariance: this solver was allocated for a block-diagonal Jacobian of %d blocks of %d x %d",
                      s->bd_blocks, s->bd_mb, s->bd_nb);
        return LSQ_EARG;
    }
    if (d_f && s->bd_mb <= s->bd_nb) {
        lsq_set_error("lsq_solver_covariance: the residual variance sum(f_b.^2) / (mb - nb) needs mb > nb (got mb = %d, nb = %d); "
                      "pass d_f = NULL for the unscaled inv(J_b'J_b)", s->bd_mb, s->bd_nb);
        return LSQ_EARG;
    }
    LSQ_HIP(hipSetDevice(c->device));
    LSQ_TRY(lsq_ensure_csc(J));        // (a device-side g! may have written the product mirrors only)
    if (!s->d_cov_info) LSQ_HIP(hipMalloc(&s->d_cov_info, (size_t)s->bd_blocks * sizeof(int)));
    if (s->bd_nb > 16) LSQ_TRY(bd_cov_launch<4>(c, J, d_f, d_cov, d_stderr, s->d_cov_info));
    else LSQ_TRY(bd_cov_launch<1>(c, J, d_f, d_cov, d_stderr, s->d_cov_info));
    if (h_info) {
        LSQ_HIP(hipMemcpyAsync(h_info, s->d_cov_info, (size_t)s->bd_blocks * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        LSQ_HIP(hipStreamSynchronize(c->stream));
    }
    return LSQ_OK;
}

extern "C" int lsq_solver_covariance(lsq_solver *s, lsq_mat *J, const double *d_f, double *d_cov, double *d_stderr,
                                     int *h_info) {
    LSQ_RANGE("lsq_solver_covariance");
    if (!s || !J) { lsq_set_error("lsq_solver_covariance: null argument"); return LSQ_EARG; }
    if (!d_cov && !d_stderr) {
        lsq_set_error("lsq_solver_covariance: d_cov and d_stderr are both NULL: nothing to compute");
        return LSQ_EARG;
    }
    if (s->kind == LSQ_SCHUR) {
        lsq_set_error("lsq_solver_covariance: not available on a Schur() solver (the covariance of a border past nb + ng = 64 is "
                      "not built). Use lsq_sparse_covariance with an LSMR() solver on the same handle, or a Cholesky() solver "
                      "when nb + ng <= 64");
        return LSQ_EARG;
    }
    if (s->kind == LSQ_BORDERED_QR) {
        lsq_set_error("lsq_solver_covariance: not available on a BorderedQR() solver (a covariance from its factors is not "
                      "built). Use lsq_sparse_covariance with an LSMR() solver on the same handle, or a Cholesky() solver "
                      "when nb + ng <= 64");
        return LSQ_EARG;
    }
    if (s->kind != LSQ_CHOLESKY || (s->bd_blocks == 0 && s->br_blocks == 0)) {
        lsq_set_error("lsq_solver_covariance: needs a Cholesky() solver created on a block-diagonal (lsq_blockdiag_create) or "
                      "bordered block-diagonal (lsq_blockdiag_bordered_create) Jacobian (this solver's kind is %d)", s->kind);
        return LSQ_EARG;
    }
    if (s->br_blocks) return lsq_bordered_covariance(s, J, d_f, d_cov, d_stderr, h_info);
    return blockdiag_covariance(s, J, d_f, d_cov, d_stderr, h_info);
}
