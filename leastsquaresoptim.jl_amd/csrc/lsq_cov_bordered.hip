// Parameter covariance from the BorderedQR() solver: lsq_bordered_qr_covariance, Cov = s^2 inv(J'J) of a bordered block-diagonal
// Jacobian J = [blkdiag(J_1 .. J_B) | C] with nb <= 64 and any ng >= 1, local-shared cross-covariances included.  Neither J'J
// nor any part of it is formed, so the condition number is not squared.
//
// With zero damping the elimination of lsq_borderedqr.hip leaves, per block, Q_b'[J_b C_b] = [R_b W_b; 0 F_b]; R of the whole
// stacked matrix is [blkdiag(R_b) W; 0 R_g] with F P = Q_g R_g, and its inverse has the blocks X_b = inv(R_b), -T_b inv(R_g)
// (T_b = inv(R_b) W_b) and inv(R_g).  With Cgg = inv(F'F):
//     Cov_gg = s^2 Cgg        Cov_bg = -s^2 T_b Cgg        Cov_bb = s^2 (X_b X_b' + (T_b Cgg) T_b')
// Stream order:
//   k_bdq_init / k_bdq_factor / k_bdq_apply   lsq_borderedqr_eliminate with a solver-owned zero damping and right-hand side
//   lsq_dense_qr_cov_factor                   the first half of lsq_dense_qr_covariance (lsq_cov_dense.hip) on the solver's inner
//                     QR() and the dense view of F, with every factorisation path and retry it has
//   -- the one wait beyond the inner QR()'s: s^2, the locals' verdict and the inner rank, read back to back --
//   lsq_dense_qr_cov_finish                   its second half: Cgg = inv(F'F) (unit variance, un-permuted) into a solver-owned
//                     ng x ng buffer
//   k_bqc_tsolve      per (block, tile of 64 border columns), the grid of k_bdq_apply: T = inv(R_b) W_b in place in the W stack.
//                     One quad of threads per column substitutes back against R_b in LDS.  (No explicit inv(R_b) here: the
//                     substitution costs the same nb^2 / 2 per column as the product with an inverse and saves forming it
//                     B ceil(ng / 64) times.)
//   k_bqc_tall        the hot path: P = T Cgg, (B nb) x ng times ng x ng, on the fp64 matrix unit with the 64 x 64 tile, the
//                     LDS staging and the fragment layout of k_cov_xxt (lsq_cov_dense.hip).  Row tiles run over the stacked
//                     rows whatever the blocks are; k runs in index order, no split.  P goes to the F stack of the solver's
//                     workspace (the inner QR() has its copy; (B mb) ng >= (B nb) ng doubles because m >= n), -s^2 P to d_cross.
//   k_bqc_block<G>    per block (16 < nb <= 64: one workgroup; nb <= 16: one wavefront, four per workgroup): X_b = inv(R_b) by
//                     the same quad substitution against the identity, then the upper S x S register tiles (S = 4 or 2) of
//                     X_b X_b' + P_b T_b', k in index order, times s^2, stored with their mirrors; the square roots of the
//                     diagonal are the local standard errors -- the same arithmetic whether d_cov is given or not.
//   k_bqc_shared      s^2 Cgg and the shared standard errors.
// No floating-point atomics, no workgroup waits for another, every sum has a fixed association.
#include <algorithm>
#include <climits>
#include <cmath>

#include "lsq_solver.h"
#include "lsq_bq.h"

constexpr int BQC_TW = 64;          // border columns per tile of k_bqc_tsolve: one per quad of the 256 threads
constexpr int BQC_T = 64;           // tile of k_bqc_tall
constexpr int BQC_KC = 32;          // k's staged per step
constexpr int BQC_KS = BQC_KC + 2;  // LDS row stride (doubles)
constexpr int BQC_BK = 16;          // k's of P_b and T_b staged per step of k_bqc_block
typedef double bqc_v4d __attribute__((ext_vector_type(4)));

// R x = w for one column w (nb entries in LDS) by the quad of threads q = 0 .. 3, in place; R: rows of an upper triangle in
// LDS, row stride ld.  Step k: thread q sums R_kj x_j over j > k, j = q (mod 4), ascending; the quad sum has a fixed shape.
// x is zero below row `top` (w = a unit vector) when top < nb - 1.  The four threads of a quad sit in one wavefront: the
// LDS traffic between them is ordered by bq_sync<1>.
__device__ __forceinline__ void bqc_quad_backsolve(const double *__restrict__ R, int ld, int nb, double *__restrict__ w, int top,
                                                   int q) {
    for (int k = top; k >= 0; --k) {
        double p = 0.0;
        for (int j = k + 1 + ((q - k - 1) & 3); j <= top; j += 4) p += R[k * ld + j] * w[j];
        p = bq_quad_sum(p);
        const double xk = (w[k] - p) / R[k * ld + k];
        bq_sync<1>();
        if (q == 0) w[k] = xk;
        bq_sync<1>();
    }
}

__global__ void __launch_bounds__(256)
k_bqc_tsolve(int B, int nb, int ng, const double *__restrict__ Rin, double *__restrict__ Wst) {
    extern __shared__ double bqc_lds[];
    const int tid = threadIdx.x, qi = tid >> 2, q = tid & 3;
    const int b = blockIdx.x, col0 = BQC_TW * (int)blockIdx.y;
    const int ld = nb | 1;
    double *sR = bqc_lds;                                  // [row][column]
    double *Wt = sR + nb * ld;                             // [column of the tile][row]
    const double *rb = Rin + (size_t)b * nb * nb;
    const size_t ldw = (size_t)B * nb;
    for (int e = tid; e < nb * nb; e += 256) {
        const int k = e / nb, c = e - k * nb;
        sR[k * ld + c] = rb[e];
    }
    const int ncol = ng - col0 < BQC_TW ? ng - col0 : BQC_TW;
    for (int e = tid; e < BQC_TW * nb; e += 256) {
        const int j = e / nb, i = e - j * nb;
        Wt[j * ld + i] = j < ncol ? Wst[(size_t)(col0 + j) * ldw + (size_t)b * nb + i] : 0.0;
    }
    __syncthreads();
    bqc_quad_backsolve(sR, ld, nb, Wt + qi * ld, nb - 1, q);
    __syncthreads();
    for (int e = tid; e < ncol * nb; e += 256) {
        const int j = e / nb, i = e - j * nb;
        Wst[(size_t)(col0 + j) * ldw + (size_t)b * nb + i] = Wt[j * ld + i];
    }
}

// Tile (blockIdx.x, blockIdx.y) of P = T Cgg: T is nr x ng, column-major with leading dimension nr; Cgg is ng x ng and symmetric
// to the bit, so its element (k, c) is read as (c, k), down a column.  Wave and fragment layout of k_cov_xxt: four wavefronts own
// the 32 x 32 quadrants, 2 x 2 MFMA 16 x 16 x 4 tiles each; operand A: lane & 15 = row, lane >> 4 = k; operand B: lane & 15 =
// column; accumulator r: row (lane >> 4) + 4 r.  P and cross (either may be null): P(row, col) and -s2 P(row, col).
__global__ void __launch_bounds__(256)
k_bqc_tall(const double *__restrict__ T, int nr, int ng, const double *__restrict__ Cgg, double s2, double *__restrict__ P,
           double *__restrict__ cross) {
    __shared__ double sA[BQC_T * BQC_KS];
    __shared__ double sB[BQC_T * BQC_KS];
    const int i0 = (int)blockIdx.x * BQC_T, j0 = (int)blockIdx.y * BQC_T;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wr = (w >> 1) * 32, wc = (w & 1) * 32;
    bqc_v4d acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = (bqc_v4d){0.0, 0.0, 0.0, 0.0};
    // staging: lane = row of T / column of the Cgg tile (coalesced down a column k), 8 k's per thread
    const int am = tid & 63, akq = (tid >> 6) * 8;
    const int ia = i0 + am, jb = j0 + am;
    const bool full = i0 + BQC_T <= nr && j0 + BQC_T <= ng;
    double ra[8], rb[8];
    auto fetch = [&](int k0) {
        if (full && k0 + BQC_KC <= ng) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int k = k0 + akq + q;
                ra[q] = T[(size_t)k * nr + ia];
                rb[q] = Cgg[(size_t)k * ng + jb];
            }
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int k = k0 + akq + q;
                ra[q] = (k < ng && ia < nr) ? T[(size_t)k * nr + ia] : 0.0;
                rb[q] = (k < ng && jb < ng) ? Cgg[(size_t)k * ng + jb] : 0.0;
            }
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < ng; k0 += BQC_KC) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            sA[am * BQC_KS + akq + q] = ra[q];
            sB[am * BQC_KS + akq + q] = rb[q];
        }
        __syncthreads();
        if (k0 + BQC_KC < ng) fetch(k0 + BQC_KC);
#pragma unroll
        for (int kk = 0; kk < BQC_KC; kk += 4) {
            const int ko = kk + (lane >> 4);
            const double a0 = sA[(wr + (lane & 15)) * BQC_KS + ko];
            const double a1 = sA[(wr + 16 + (lane & 15)) * BQC_KS + ko];
            const double b0 = sB[(wc + (lane & 15)) * BQC_KS + ko];
            const double b1 = sB[(wc + 16 + (lane & 15)) * BQC_KS + ko];
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
                if (row < nr && col < ng) {
                    const double v = acc[a][b][r];
                    const size_t o = (size_t)col * nr + row;
                    if (P) P[o] = v;
                    if (cross) cross[o] = -(s2 * v);
                }
            }
}

// Block b: Cov_bb = s2 (X_b X_b' + P_b T_b') and the local standard errors.  Thread (ti, tj) of the group owns the S x S
// entries (S ti + a, S tj + c); tiles below the diagonal stay idle, the mirrors are stored from the upper ones.
template <int G>
__global__ void __launch_bounds__(256)
k_bqc_block(int B, int nb, int ng, const double *__restrict__ Rin, const double *__restrict__ Tst, const double *__restrict__ Pst,
            double s2, double *__restrict__ cov, double *__restrict__ se, size_t group_doubles) {
    extern __shared__ double bqc_lds[];
    constexpr int GT = 64 * G, NQ = 16 * G;                // threads and quads per block
    constexpr int S = G == 4 ? 4 : 2, NP = G == 4 ? 64 : 16, TPR = NP / S;   // register tile, padded nb, tiles per row
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int gt = G == 4 ? tid : lane;
    const int b = G == 4 ? (int)blockIdx.x : (int)blockIdx.x * 4 + wv;
    if (b >= B) return;                // (G == 1: the wavefronts of a workgroup never meet at a barrier)
    const int ld = nb | 1;
    double *sX = bqc_lds + (G == 4 ? 0 : wv) * group_doubles;      // [column c][row i] of X_b = inv(R_b), NQ columns
    double *sR = sX + NQ * ld;                                    // [row][column]; afterwards the staging of P_b and T_b
    double *sP = sR, *sT = sR + BQC_BK * NP;                      // [k][row of the block]
    const double *rb = Rin + (size_t)b * nb * nb;
    for (int e = gt; e < nb * nb; e += GT) {
        const int k = e / nb, c = e - k * nb;
        sR[k * ld + c] = rb[e];
    }
    for (int e = gt; e < NQ * ld; e += GT) {
        const int c = e / ld, i = e - c * ld;
        sX[e] = c == i ? 1.0 : 0.0;
    }
    bq_sync<G>();
    const int qi = gt >> 2, q = gt & 3;
    if (qi < nb) bqc_quad_backsolve(sR, ld, nb, sX + qi * ld, qi, q);
    bq_sync<G>();
    const int ti = gt / TPR, tj = gt - ti * TPR;
    const bool on = ti <= tj && S * tj < nb;
    double acc[S][S];
#pragma unroll
    for (int a = 0; a < S; ++a)
#pragma unroll
        for (int c = 0; c < S; ++c) acc[a][c] = 0.0;
    if (on) {                          // X X': column k of X is sX[k ld + .], zero below row k; k in index order
        for (int k = S * tj; k < nb; ++k) {
            double xa[S], xc[S];
#pragma unroll
            for (int a = 0; a < S; ++a) {
                const int i = S * ti + a, j = S * tj + a;
                xa[a] = i < nb ? sX[k * ld + i] : 0.0;
                xc[a] = j < nb ? sX[k * ld + j] : 0.0;
            }
#pragma unroll
            for (int a = 0; a < S; ++a)
#pragma unroll
                for (int c = 0; c < S; ++c) acc[a][c] += xa[a] * xc[c];
        }
    }
    bq_sync<G>();                      // sR is free: the staging stands there
    const size_t ldw = (size_t)B * nb, rbase = (size_t)b * nb;
    for (int k0 = 0; k0 < ng; k0 += BQC_BK) {
        for (int e = gt; e < BQC_BK * NP; e += GT) {
            const int kk = e / NP, i = e - kk * NP;
            const bool in = i < nb && k0 + kk < ng;
            const size_t o = (size_t)(k0 + kk) * ldw + rbase + i;
            sP[e] = in ? Pst[o] : 0.0;
            sT[e] = in ? Tst[o] : 0.0;
        }
        bq_sync<G>();
        if (on) {
#pragma unroll 4
            for (int kk = 0; kk < BQC_BK; ++kk) {
                double pa[S], tc[S];
#pragma unroll
                for (int a = 0; a < S; ++a) {
                    pa[a] = sP[kk * NP + S * ti + a];
                    tc[a] = sT[kk * NP + S * tj + a];
                }
#pragma unroll
                for (int a = 0; a < S; ++a)
#pragma unroll
                    for (int c = 0; c < S; ++c) acc[a][c] += pa[a] * tc[c];
            }
        }
        bq_sync<G>();                  // the next k's are staged over these
    }
    if (!on) return;
    double *cb = cov ? cov + (size_t)b * nb * nb : nullptr;
    double *sb = se ? se + (size_t)b * nb : nullptr;
#pragma unroll
    for (int a = 0; a < S; ++a)
#pragma unroll
        for (int c = 0; c < S; ++c) {
            const int i = S * ti + a, j = S * tj + c;
            if (i <= j && j < nb) {
                const double v = s2 * acc[a][c];
                if (cb) {
                    cb[(size_t)i * nb + j] = v;
                    cb[(size_t)j * nb + i] = v;
                }
                if (sb && i == j) sb[i] = sqrt(v);
            }
        }
}

// covg (ng x ng) = s2 Cgg, seg = sqrt of its diagonal; either may be null
__global__ void __launch_bounds__(256)
k_bqc_shared(int ng, const double *__restrict__ Cgg, double s2, double *__restrict__ covg, double *__restrict__ seg) {
    const long long tot = (long long)ng * ng;
    for (long long e = blockIdx.x * 256LL + threadIdx.x; e < tot; e += (long long)gridDim.x * 256) {
        const double v = s2 * Cgg[e];
        if (covg) covg[e] = v;
        if (seg && e % ng == e / ng) seg[e / ng] = sqrt(v);
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// doubles of LDS per block of k_bqc_block: X (NQ columns of nb | 1) | R (nb rows of nb | 1), later 2 BQC_BK rows of NP
static size_t bqc_block_doubles(int nb, int G) {
    const size_t ld = (size_t)(nb | 1), r = (size_t)nb * ld, stage = 2 * (size_t)BQC_BK * (G == 4 ? 64 : 16);
    return (size_t)(16 * G) * ld + (r > stage ? r : stage);
}

template <int G>
static int bqc_block(lsq_ctx *c, lsq_solver *s, const double *R, const double *T, const double *P, double s2, double *d_cov,
                     double *d_stderr) {
    const int B = s->br_blocks;
    const size_t gd = bqc_block_doubles(s->br_nb, G);
    const size_t lds = (G == 4 ? 1 : 4) * gd * sizeof(double);
    LSQ_TRY(lsq_set_lds(c, (const void *)k_bqc_block<G>, lds));
    LSQ_LAUNCH((k_bqc_block<G>), dim3(G == 4 ? B : (B + 3) / 4), dim3(256), lds, c->stream, B, s->br_nb, s->br_ng, R, T, P, s2,
               d_cov, d_stderr, gd);
    return LSQ_OK;
}

extern "C" int lsq_bordered_qr_covariance(lsq_solver *s, lsq_mat *J, const double *d_f, double *d_cov, double *d_stderr,
                                          double *d_cross, int *h_info) {
    LSQ_RANGE("lsq_bordered_qr_covariance");
    if (!s || !J) { lsq_set_error("lsq_bordered_qr_covariance: null argument"); return LSQ_EARG; }
    if (!d_cov && !d_stderr && !d_cross) {
        lsq_set_error("lsq_bordered_qr_covariance: d_cov, d_stderr and d_cross are all NULL: nothing to compute");
        return LSQ_EARG;
    }
    if (s->kind != LSQ_BORDERED_QR || !s->inner || !s->inner_J) {
        lsq_set_error("lsq_bordered_qr_covariance: needs a BorderedQR() solver created on a bordered block-diagonal Jacobian "
                      "(lsq_blockdiag_bordered_create); this solver's kind is %d (a Cholesky() solver on such a handle has "
                      "lsq_solver_covariance, an LSMR() solver lsq_sparse_covariance, a dense QR() solver lsq_dense_qr_covariance)",
                      s->kind);
        return LSQ_EARG;
    }
    if (J->kind != LSQ_MAT_CSC || J->br_blocks < 1) {
        const char *what = J->kind == LSQ_MAT_DENSE ? "a dense handle (lsq_dense_create): lsq_dense_qr_covariance serves it"
                           : J->kind != LSQ_MAT_CSC ? "an operator handle (lsq_op_create): no covariance is offered for it"
                           : J->bd_blocks > 0       ? "a block-diagonal handle without shared columns (lsq_blockdiag_create): "
                                                      "lsq_solver_covariance serves it"
                                                    : "a plain CSC handle (lsq_csc_create): lsq_sparse_covariance serves it";
        lsq_set_error("lsq_bordered_qr_covariance: the Jacobian is not a bordered block-diagonal handle "
                      "(lsq_blockdiag_bordered_create); this is %s", what);
        return LSQ_EARG;
    }
    if (J->br_blocks != s->br_blocks || J->br_mb != s->br_mb || J->br_nb != s->br_nb || J->br_ng != s->br_ng || J->m != s->m ||
        J->n != s->n) {
        lsq_set_error("lsq_bordered_qr_covariance: this solver was allocated for a bordered block-diagonal Jacobian of %d blocks "
                      "of %d x %d with %d shared columns; create a solver on the handle whose covariance is wanted", s->br_blocks,
                      s->br_mb, s->br_nb, s->br_ng);
        return LSQ_EARG;
    }
    const int m = J->m, n = J->n;
    if (m < n) {
        lsq_set_error("lsq_bordered_qr_covariance: inv(J'J) needs m >= n (got m = %d, n = %d); a pseudo-inverse covariance is "
                      "not offered", m, n);
        return LSQ_EARG;
    }
    if (d_f && m <= n) {
        lsq_set_error("lsq_bordered_qr_covariance: the residual variance sum(f.^2) / (m - n) needs m > n (got m = %d, n = %d); "
                      "pass d_f = NULL for the unscaled inv(J'J)", m, n);
        return LSQ_EARG;
    }
    if (h_info) h_info[0] = h_info[1] = 0;
    lsq_ctx *c = s->ctx;
    LSQ_HIP(hipSetDevice(c->device));
    LSQ_TRY(lsq_ensure_csc(J));        // (a device-side g! may have written the product mirrors only)
    const int B = s->br_blocks, nb = s->br_nb, ng = s->br_ng;
    // zeros: the right-hand side (m) and the damping (n <= m) of the elimination | Cgg (ng x ng)
    if (!s->d_cov_buf) {
        LSQ_HIP(hipMalloc(&s->d_cov_buf, ((size_t)m + (size_t)ng * ng) * sizeof(double)));
        LSQ_HIP(hipMemsetAsync(s->d_cov_buf, 0, (size_t)m * sizeof(double), c->stream));
    }
    const double *zero = s->d_cov_buf;
    double *Cgg = s->d_cov_buf + m;
    LsqBdqView v;
    LSQ_TRY(lsq_borderedqr_eliminate(s, J, zero, zero, &v));
    s->last_bd_path = 6;
    s->last_bd_block = -1;
    const double *Xg = nullptr;
    const int *jp = nullptr;
    LSQ_TRY(lsq_dense_qr_cov_factor(s->inner, s->inner_J, &Xg, &jp));
    // the one wait beyond the inner QR()'s: the variance and, behind it, the verdict on the locals and the inner rank
    double ssq = 0.0;
    int st4[4] = {0, 0, 0, 0};
    if (d_f) LSQ_TRY(lsq_sumsq(c, m, d_f, &ssq));
    LSQ_TRY(lsq_read_ints(c, s->d_info, s->inner->d_info, nullptr, nullptr, st4));
    const int rank = st4[1];
    s->inner->last_rank = rank;
    if (h_info) h_info[1] = rank;
    if (st4[0] != INT_MAX) {
        s->last_bd_block = (st4[0] - 1) / nb;
        if (h_info) h_info[0] = st4[0];
        lsq_set_error("RankDeficientException: BorderedQR(): the triangular factor of the local columns has a zero or non-finite "
                      "diagonal entry at column %d (a zero damping value on a zero column, or a non-finite operand)", st4[0]);
        return LSQ_ERANK;
    }
    if (rank < ng) {
        lsq_set_error("RankDeficientException(%d): lsq_bordered_qr_covariance: the transformed border of the shared columns has "
                      "rank %d < ng = %d (xGELSY's decision at rcond = ng eps); a pseudo-inverse covariance is not offered",
                      rank, rank, ng);
        return LSQ_ERANK;
    }
    const double s2 = d_f ? ssq / (double)(m - n) : 1.0;
    const int nr = B * nb;
    LSQ_TRY(lsq_dense_qr_cov_finish(s->inner, ng, Xg, jp, 1.0, Cgg, nullptr));       // Cgg = inv(F'F), un-permuted
    const size_t lds_t = ((size_t)nb * (nb | 1) + (size_t)BQC_TW * (nb | 1)) * sizeof(double);
    LSQ_TRY(lsq_set_lds(c, (const void *)k_bqc_tsolve, lds_t));
    LSQ_LAUNCH(k_bqc_tsolve, dim3(B, lsq_div_up(ng, BQC_TW)), dim3(256), lds_t, c->stream, B, nb, ng, (const double *)v.R, v.W);
    const bool locals = d_cov || d_stderr;          // (P itself is read by the per-block kernel only)
    LSQ_LAUNCH(k_bqc_tall, dim3(lsq_div_up(nr, BQC_T), lsq_div_up(ng, BQC_T)), dim3(256), 0, c->stream, (const double *)v.W, nr,
               ng, (const double *)Cgg, s2, locals ? v.F : (double *)nullptr, d_cross);
    if (locals) {
        if (nb > 16) LSQ_TRY(bqc_block<4>(c, s, v.R, v.W, v.F, s2, d_cov, d_stderr));
        else LSQ_TRY(bqc_block<1>(c, s, v.R, v.W, v.F, s2, d_cov, d_stderr));
        const long long tot = (long long)ng * ng;
        const int g = (int)std::min<long long>((tot + 255) / 256, (long long)c->num_cus * 8);
        LSQ_LAUNCH(k_bqc_shared, dim3(g), dim3(256), 0, c->stream, ng, (const double *)Cgg, s2,
                   d_cov ? d_cov + (size_t)B * nb * nb : (double *)nullptr, d_stderr ? d_stderr + (size_t)nr : (double *)nullptr);
    }
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}
