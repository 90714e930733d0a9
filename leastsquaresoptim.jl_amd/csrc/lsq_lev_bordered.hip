// Leverages and prediction variances of a bordered block-diagonal fit from the BorderedQR() factor: lsq_bordered_qr_leverage,
// q(a) = a' inv(J'J) a for the rows of J = [blkdiag(J_1 .. J_B) | C] itself or for new rows of one block, nb <= 64, any ng >= 1.
// Neither J'J nor the n x n covariance is formed.
//
// With zero damping the elimination of lsq_borderedqr.hip leaves, per block, Q_b'[J_b C_b] = [R_b W_b; 0 F_b], and the stacked F
// factors as F P = Q_g R_g (the solver's inner QR()).  A row of block b with local part a_b (nb) and shared part c (ng):
//     z = inv(R_b)' a_b        e = c - W_b' z        u = inv(R_g)' P' e        q = ||z||^2 + ||u||^2
// (for the rows of J_b itself E = C_b - (J_b inv(R_b)) W_b = Q_b2 F_b).  Stream order:
//   k_bdq_init / k_bdq_factor / k_bdq_apply   lsq_borderedqr_eliminate with the solver-owned zero damping and right-hand side
//   lsq_dense_qr_cov_factor                   X_g = inv(R_g) and the pivots of the inner QR() (lsq_cov_dense.hip)
//   -- the one wait beyond the inner QR()'s: s^2, the locals' verdict and the inner rank, read back to back --
//   k_bl_local     one 256-thread workgroup per (block, slab of 64 rows); a slab never straddles two blocks.  R_b is staged in
//                  LDS; the slab of A_b goes into LDS row by row (the handle's column scale applied on the way, as
//                  k_bdq_factor does) and one quad of threads per row substitutes forward against R_b in place: thread q sums
//                  z_j R_jk over j < k, j = q (mod 4), ascending, the quad sum has a fixed shape.  Z = A_b inv(R_b) stays
//                  resident; qz_i = ||z_i||^2 is summed in index order by the quad's first thread.  Then, for every tile of 64
//                  border columns, P = Z W_b[:, tile] on the fp64 matrix unit -- the 64 x 64 tile, the k-chunks of 32 for the
//                  staging of W_b, the wave and fragment layout of k_lev_tall and k_bqc_tall; k in index order over nb padded
//                  to a multiple of 4, no split -- goes through LDS (over the place of R_b, which is no longer needed) so that
//                  C is read and E = C - P is written down the columns: (rows) x ng, column-major.  Rows past the block's
//                  last, columns past ng and k past nb are taken as 0.  W is left as the elimination wrote it.
//                  For J's own rows E goes into the F stack of the solver's workspace (the inner QR() has its copy), for new
//                  rows into the solver's leverage scratch.  LDS: 64 x 65 (R_b / P) + 64 x (nb4 + 2) (Z) + 64 x 34 (W tile)
//                  doubles, 82.5 KiB at nb = 64: one workgroup per CU.  blockIdx.y: a group of border tiles; every group
//                  forms Z again, from the same operands in the same order, so the grouping changes no bits.
//   k_lev_tall     (lsq_leverage.hip) on E with X = X_g, the inner pivots and n = ng: qg_i = ||X_g' P' e_i||^2
//   k_bl_add       q_i = qz_i + qg_i, one IEEE addition
//   k_lev_diag     (lsq_leverage.hip) se, t, cook with the one variance and ncook = n = B nb + ng
// No floating-point atomics, no workgroup waits for another, every sum has a fixed association; row i's bits depend on row i,
// R_b, W_b and X_g only -- not on p, on the slab or the position inside it, on the other rows, on the run or the launch mode.
#include <algorithm>
#include <climits>
#include <cmath>

#include "lsq_solver.h"
#include "lsq_bq.h"

constexpr int BLV_T = 64;             // rows per slab, border columns per tile
constexpr int BLV_KC = 32;            // k's of W_b staged per step
constexpr int BLV_KS = BLV_KC + 2;    // LDS row stride of the staged W tile (doubles)
constexpr int BLV_PS = BLV_T + 1;     // LDS column stride of the P tile (doubles)
typedef double blv_v4d __attribute__((ext_vector_type(4)));

// doubles of LDS: R_b (nb rows of nb | 1 <= 64 x 65), later the P tile (64 columns of 65) | Z (64 rows of nb4 + 2) | W tile
static inline size_t blv_doubles(int nb) {
    const size_t nb4 = (size_t)((nb + 3) & ~3);
    return (size_t)BLV_T * BLV_PS + (size_t)BLV_T * (nb4 + 2) + (size_t)BLV_T * BLV_KS;
}

// Workgroup blockIdx.x = (data block db, slab); bfix < 0: the factor's block is db (J's own rows), else bfix with db = 0 (new
// rows).  Al: the local parts, block db at Al + db al_bs, column-major with leading dimension lda; Ag: the shared parts
// likewise (ag_bs, ldg); `rows` rows per data block.  scale: null, or the handle's n factors (sg0 = B nb: where the shared
// ones start).  Rin: R_b as rows (nb x nb per block); Wst: the W stack, column-major with leading dimension ldw = B nb.
// E (block db at E + db e_bs, leading dimension lde) and qz (block db at qz + db e_bs) are the outputs; qz may be null.
__global__ void __launch_bounds__(256)
k_bl_local(int slabs, int rows, int nb, int ng, int ldw, int bfix, const double *__restrict__ Al, size_t al_bs, int lda,
           const double *__restrict__ Ag, size_t ag_bs, int ldg, const double *__restrict__ scale, int sg0,
           const double *__restrict__ Rin, const double *__restrict__ Wst, double *__restrict__ E, size_t e_bs, int lde,
           double *__restrict__ qz, int tpg) {
    extern __shared__ double blv_lds[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int db = (int)blockIdx.x / slabs, r0 = ((int)blockIdx.x - db * slabs) * BLV_T;
    const int b = bfix >= 0 ? bfix : db;
    const int ld = nb | 1, nb4 = (nb + 3) & ~3, zs = nb4 + 2;
    double *sR = blv_lds;                          // [row][column]
    double *sP = blv_lds;                          // [column of the tile][row of the slab], once Z stands
    double *sZ = blv_lds + BLV_T * BLV_PS;         // [row of the slab][k]
    double *sB = sZ + BLV_T * zs;                  // [column of the tile][k of the chunk]
    const double *rb = Rin + (size_t)b * nb * nb;
    for (int e = tid; e < nb * nb; e += 256) {
        const int k = e / nb, c = e - k * nb;
        sR[k * ld + c] = rb[e];
    }
    // the slab of A_b: lane = row (coalesced down a column)
    const int am = tid & 63, ia = r0 + am;
    const bool arow = ia < rows;
    const double *al = Al + (size_t)db * al_bs;
    for (int k = w; k < nb4; k += 4) {
        double v = 0.0;
        if (arow && k < nb) {
            v = al[(size_t)k * lda + ia];
            if (scale) v = v * scale[(size_t)b * nb + k];
        }
        sZ[am * zs + k] = v;
    }
    __syncthreads();
    // z' R_b = a': one quad per row, in place
    {
        const int qi = tid >> 2, q = tid & 3;
        double *z = sZ + qi * zs;
        for (int k = 0; k < nb; ++k) {
            double p = 0.0;
            for (int j = q; j < k; j += 4) p += sR[j * ld + k] * z[j];
            p = bq_quad_sum(p);
            const double zk = (z[k] - p) / sR[k * ld + k];
            bq_sync<1>();
            if (q == 0) z[k] = zk;
            bq_sync<1>();
        }
        if (q == 0 && qz && blockIdx.y == 0 && r0 + qi < rows) {
            double s = 0.0;
            for (int k = 0; k < nb; ++k) s = s + z[k] * z[k];
            qz[(size_t)db * e_bs + r0 + qi] = s;
        }
    }
    __syncthreads();                               // Z stands; R_b is not read again

    const int wr = (w >> 1) * 32, wc = (w & 1) * 32;
    const int bk = tid & 31, bc = tid >> 5;        // staging of W_b: lane & 31 = k (coalesced down a column), 8 columns per thread
    const double *ag = Ag + (size_t)db * ag_bs;
    double *eo = E + (size_t)db * e_bs;
    const double *wb = Wst + (size_t)b * nb;
    const int nt = (ng + BLV_T - 1) / BLV_T;
    const int t0 = (int)blockIdx.y * tpg, t1 = t0 + tpg < nt ? t0 + tpg : nt;
    for (int t = t0; t < t1; ++t) {
        const int j0 = t * BLV_T;
        // the slab's rows of C for this tile, in flight during the product: lane = row, columns w, w + 4, ..
        double cr[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int gc = j0 + w + 4 * u;
            double v = 0.0;
            if (arow && gc < ng) {
                v = ag[(size_t)gc * ldg + ia];
                if (scale) v = v * scale[(size_t)sg0 + gc];
            }
            cr[u] = v;
        }
        blv_v4d acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int c = 0; c < 2; ++c) acc[a][c] = (blv_v4d){0.0, 0.0, 0.0, 0.0};
        double rw[8];
        auto fetch = [&](int k0) {
            const int k = k0 + bk;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int gc = j0 + bc + 8 * u;
                rw[u] = (gc < ng && k < nb) ? wb[(size_t)gc * ldw + k] : 0.0;
            }
        };
        fetch(0);
        for (int k0 = 0; k0 < nb4; k0 += BLV_KC) {
#pragma unroll
            for (int u = 0; u < 8; ++u) sB[(bc + 8 * u) * BLV_KS + bk] = rw[u];
            __syncthreads();
            if (k0 + BLV_KC < nb4) fetch(k0 + BLV_KC);
            const int kn = nb4 - k0 < BLV_KC ? nb4 - k0 : BLV_KC;
            for (int kk = 0; kk < kn; kk += 4) {
                const int ko = kk + (lane >> 4);
                const double a0 = sZ[(wr + (lane & 15)) * zs + k0 + ko];
                const double a1 = sZ[(wr + 16 + (lane & 15)) * zs + k0 + ko];
                const double b0 = sB[(wc + (lane & 15)) * BLV_KS + ko];
                const double b1 = sB[(wc + 16 + (lane & 15)) * BLV_KS + ko];
                acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
            }
            __syncthreads();
        }
        // P through LDS: accumulator r of (a, c) is row wr + 16 a + (lane >> 4) + 4 r, column wc + 16 c + (lane & 15)
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    sP[(wc + c * 16 + (lane & 15)) * BLV_PS + wr + a * 16 + (lane >> 4) + 4 * r] = acc[a][c][r];
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int cc = w + 4 * u, gc = j0 + cc;
            if (arow && gc < ng) eo[(size_t)gc * lde + ia] = cr[u] - sP[cc * BLV_PS + am];
        }
        __syncthreads();                           // the next tile's P is written over this one
    }
}

// q = qz + qg
__global__ void __launch_bounds__(256)
k_bl_add(long long n, const double *__restrict__ qz, const double *__restrict__ qg, double *__restrict__ q) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) q[i] = qz[i] + qg[i];
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
extern "C" int lsq_bordered_qr_leverage(lsq_solver *s, lsq_mat *J, int block, const double *d_Ab, int ldab, const double *d_Ag,
                                        int ldag, int p, const double *d_f, double *d_q, double *d_se, double *d_student,
                                        double *d_cook, double *h_s2, int *h_info) {
    LSQ_RANGE("lsq_bordered_qr_leverage");
    if (!s || !J) { lsq_set_error("lsq_bordered_qr_leverage: null argument"); return LSQ_EARG; }
    if (!d_q && !d_se && !d_student && !d_cook && !h_s2) {
        lsq_set_error("lsq_bordered_qr_leverage: d_q, d_se, d_student, d_cook and h_s2 are all NULL: nothing to compute");
        return LSQ_EARG;
    }
    if (s->kind != LSQ_BORDERED_QR || !s->inner || !s->inner_J) {
        lsq_set_error("lsq_bordered_qr_leverage: needs a BorderedQR() solver created on a bordered block-diagonal Jacobian "
                      "(lsq_blockdiag_bordered_create); this solver's kind is %d (a QR() solver on a dense handle has "
                      "lsq_dense_qr_leverage, a Cholesky() solver on a block-diagonal handle lsq_solver_leverage)", s->kind);
        return LSQ_EARG;
    }
    if (J->kind != LSQ_MAT_CSC || J->br_blocks < 1) {
        const char *what = J->kind == LSQ_MAT_DENSE ? "a dense handle (lsq_dense_create): lsq_dense_qr_leverage serves it"
                           : J->kind != LSQ_MAT_CSC ? "an operator handle (lsq_op_create): no leverages are offered for it"
                           : J->bd_blocks > 0       ? "a block-diagonal handle without shared columns (lsq_blockdiag_create): "
                                                      "lsq_solver_leverage serves it"
                                                    : "a plain CSC handle (lsq_csc_create): no leverages are offered for it, "
                                                      "lsq_sparse_covariance gives the parameter covariance";
        lsq_set_error("lsq_bordered_qr_leverage: the Jacobian is not a bordered block-diagonal handle "
                      "(lsq_blockdiag_bordered_create); this is %s", what);
        return LSQ_EARG;
    }
    if (J->br_blocks != s->br_blocks || J->br_mb != s->br_mb || J->br_nb != s->br_nb || J->br_ng != s->br_ng || J->m != s->m ||
        J->n != s->n) {
        lsq_set_error("lsq_bordered_qr_leverage: this solver was allocated for a bordered block-diagonal Jacobian of %d blocks "
                      "of %d x %d with %d shared columns; create a solver on the handle whose leverages are wanted", s->br_blocks,
                      s->br_mb, s->br_nb, s->br_ng);
        return LSQ_EARG;
    }
    const int m = J->m, n = J->n;
    const int B = s->br_blocks, mb = s->br_mb, nb = s->br_nb, ng = s->br_ng;
    if (m < n) {
        lsq_set_error("lsq_bordered_qr_leverage: inv(J'J) needs m >= n (got m = %d, n = %d); a pseudo-inverse is not offered", m, n);
        return LSQ_EARG;
    }
    if (d_f && m <= n) {
        lsq_set_error("lsq_bordered_qr_leverage: the residual variance sum(f.^2) / (m - n) needs m > n (got m = %d, n = %d); "
                      "pass d_f = NULL for the quadratic forms alone", m, n);
        return LSQ_EARG;
    }
    if (!d_f && (d_se || d_student || d_cook || h_s2)) {
        lsq_set_error("lsq_bordered_qr_leverage: d_se, d_student, d_cook and h_s2 need the residual d_f (s^2 = sum(f.^2) / (m - n)); "
                      "without it only d_q is available");
        return LSQ_EARG;
    }
    if ((d_Ab == nullptr) != (d_Ag == nullptr)) {
        lsq_set_error("lsq_bordered_qr_leverage: new rows need both parts, d_Ab (p x nb, the block's local columns) and d_Ag "
                      "(p x ng, the shared columns); pass both NULL for the rows of J itself");
        return LSQ_EARG;
    }
    const bool fresh = d_Ab != nullptr;
    if (fresh && (d_student || d_cook)) {
        lsq_set_error("lsq_bordered_qr_leverage: d_student and d_cook belong to the rows of J itself (they pair q_i with f_i); "
                      "with new rows d_Ab / d_Ag they must be NULL");
        return LSQ_EARG;
    }
    if (fresh && (block < 0 || block >= B)) {
        lsq_set_error("lsq_bordered_qr_leverage: new rows belong to one block, 0 <= block < B = %d (got block = %d); rows of "
                      "several blocks take one call per block", B, block);
        return LSQ_EARG;
    }
    if (fresh && (p < 1 || ldab < p || ldag < p)) {
        lsq_set_error("lsq_bordered_qr_leverage: d_Ab is p x nb and d_Ag p x ng, column-major, and need p >= 1, ldab >= p and "
                      "ldag >= p (got p = %d, ldab = %d, ldag = %d)", p, ldab, ldag);
        return LSQ_EARG;
    }
    if (h_info) h_info[0] = h_info[1] = 0;
    lsq_ctx *c = s->ctx;
    LSQ_HIP(hipSetDevice(c->device));
    LSQ_TRY(lsq_ensure_csc(J));        // (a device-side g! may have written the product mirrors only)
    // zeros: the right-hand side (m) and the damping (n <= m) of the elimination | lsq_bordered_qr_covariance's Cgg (ng x ng)
    if (!s->d_cov_buf) {
        LSQ_HIP(hipMalloc(&s->d_cov_buf, ((size_t)m + (size_t)ng * ng) * sizeof(double)));
        LSQ_HIP(hipMemsetAsync(s->d_cov_buf, 0, (size_t)m * sizeof(double), c->stream));
    }
    const double *zero = s->d_cov_buf;
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
        lsq_set_error("RankDeficientException(%d): lsq_bordered_qr_leverage: the transformed border of the shared columns has "
                      "rank %d < ng = %d (xGELSY's decision at rcond = ng eps); a pseudo-inverse covariance is not offered",
                      rank, rank, ng);
        return LSQ_ERANK;
    }
    const double s2 = d_f ? ssq / (double)(m - n) : 1.0;
    if (h_s2) *h_s2 = s2;
    if (!d_q && !d_se && !d_student && !d_cook) return LSQ_OK;
    // scratch: qz | qg | q (when the caller does not take it) | E (new rows)
    const size_t rows = fresh ? (size_t)p : (size_t)m;
    double *buf = nullptr;
    LSQ_TRY(lsq_lev_scratch(s, 2 * rows + (d_q ? 0 : rows) + (fresh ? rows * (size_t)ng : 0), &buf));
    double *qz = buf, *qg = buf + rows;
    double *q = d_q ? d_q : buf + 2 * rows;
    double *E = fresh ? buf + 2 * rows + (d_q ? 0 : rows) : v.F;
    const int per = fresh ? p : mb;                                  // rows per data block
    const int slabs = lsq_div_up(per, BLV_T);
    const long long wgs = (long long)slabs * (fresh ? 1 : B);
    // too few workgroups for the chip: groups of border tiles in the second grid dimension
    const int nt = lsq_div_up(ng, BLV_T);
    int groups = (int)std::min<long long>(nt, std::max<long long>(1, c->num_cus / wgs));
    const int tpg = lsq_div_up(nt, groups);
    groups = lsq_div_up(nt, tpg);
    const size_t lds = blv_doubles(nb) * sizeof(double);
    LSQ_TRY(lsq_set_lds(c, (const void *)k_bl_local, lds));
    if (fresh) {
        LSQ_LAUNCH(k_bl_local, dim3((unsigned)wgs, groups), dim3(256), lds, c->stream, slabs, per, nb, ng, B * nb, block, d_Ab,
                   (size_t)0, ldab, d_Ag, (size_t)0, ldag, (const double *)nullptr, B * nb, (const double *)v.R,
                   (const double *)v.W, E, (size_t)0, p, qz, tpg);
    } else {
        const double *vals = J->csc.d_val;
        LSQ_LAUNCH(k_bl_local, dim3((unsigned)wgs, groups), dim3(256), lds, c->stream, slabs, per, nb, ng, B * nb, -1, vals,
                   (size_t)mb * nb, mb, vals + (size_t)m * nb, (size_t)mb, m, J->d_colscale, B * nb, (const double *)v.R,
                   (const double *)v.W, E, (size_t)mb, m, qz, tpg);
    }
    LSQ_LAUNCH(k_lev_tall, dim3(lsq_div_up((long long)rows, 64)), dim3(256), 0, c->stream, (const double *)E, (int)rows, (int)rows,
               ng, Xg, jp, (const double *)nullptr, qg);
    LSQ_LAUNCH(k_bl_add, dim3(lsq_div_up((long long)rows, 256)), dim3(256), 0, c->stream, (long long)rows, (const double *)qz,
               (const double *)qg, q);
    if (d_se || d_student || d_cook)
        LSQ_LAUNCH(k_lev_diag, dim3(lsq_div_up((long long)rows, 256)), dim3(256), 0, c->stream, (long long)rows, (const double *)q,
                   d_f, s2, (const double *)nullptr, 1, (double)n, d_se, d_student, d_cook);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}
