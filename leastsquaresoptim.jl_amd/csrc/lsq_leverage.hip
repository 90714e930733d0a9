// Leverages and prediction variances: the quadratic form q(a) = a' inv(J'J) a for the rows of J itself (q_i = h_i, the diagonal
// of the hat matrix) or for new rows, and what is derived from it and the residual -- standard errors of a prediction,
// internally studentized residuals, Cook's distances.
//
// lsq_dense_qr_leverage (dense handle, QR() solver): the factor is lsq_dense_qr_covariance's (lsq_dense_qr_cov_factor,
// lsq_cov_dense.hip): X = inv(R) and the pivots jp of J P = Q R stand on the device.  q(a) = ||X' P' a||^2:
//   k_lev_tall   the hot path.  One 256-thread workgroup per 64-row slab of A.  For each 64-column tile Jt of X in index order:
//                Z[:, Jt] = sum_{K <= Jt} A[:, jp[K]] X[K, Jt] on the fp64 matrix unit -- the 64 x 64 tile, the k-chunks of 32, the
//                LDS staging and the fragment layout of k_cov_xxt (lsq_cov_dense.hip) and k_bqc_tall (lsq_cov_bordered.hip) -- and
//                the squares of the accumulators go straight into per-lane row sums; Z is never written to memory.  Only K <= Jt
//                contributes (X is upper triangular); on the way into LDS element (k, c) of X is taken as 0 unless k <= c < n --
//                tri_X is never written below its diagonal and may hold NaN there -- and A as 0 for rows past p and k's past the
//                tile's last.  The permutation and the column scale are applied while A is staged.  The slab of A is 512 n bytes
//                (1 MiB at n = 2048), so it is not kept in LDS: every column tile stages its k-chunks again, from L2, and the
//                workgroup stays at 35 KiB of LDS (four per CU).  X is read once per slab.
//                k runs in index order with no split; a lane adds the squares of its columns tile after tile in index order,
//                a fixed butterfly adds the 16 lanes of a row, the two wavefronts that share a row are added in a fixed order: no
//                floating-point atomics, no workgroup waits for another, and row i's bits depend on row i and X only -- not
//                on p, on the slab or the position inside it, on the other rows, on the run or on the launch mode.
//   k_lev_diag   elementwise, (q, f, s2) -> se, t, cook in the operation order include/lsqhip.h fixes.  Every line is one IEEE
//                operation (the build has -ffp-contract=off; f64 sqrt and division are correctly rounded), so a numpy twin
//                reproduces the bits.
// lsq_solver_leverage (block-diagonal handle, Cholesky() solver): one independent fit per block.
//   k_bd_lev<G>  the geometry and steps 1-2 of k_bd_cov (lsq_cov.hip; restated here, so that k_bd_cov compiles to what it did):
//                streaming Gram and sum(f_b.^2), G_b = U'U, Y = inv(U)' in LDS.  ||Y a_i||^2 from that factor alone carries
//                cond(J_b)^2 u -- on blocks with cond 1e3 it misses the accuracy tier's rule against a QR reference by 15 to
//                215 x -- so the kernel is a CholeskyQR2: a second pass over the block's rows, 32 at a time, lanes down a
//                column of J_b (coalesced loads), forms z_i = Y a_i (Y read from LDS as a broadcast, k in index order) and the
//                Gram matrix G2 = sum z z' on the matrix unit exactly as the first pass forms G_b; G2 = U2'U2, Y2 = inv(U2)'
//                by the same routines (G2 is the identity up to cond(G_b) u, so this factorisation is harmless); a third pass
//                forms z_i again and h_i = ||Y2 z_i||^2 -- each of the CP threads of a row adds the squares of its entries in
//                index order, the CP partial sums are added in index order.  J_b = (Q1 inv(U2)) (U2 U) with the first factor
//                orthonormal to rounding: the accuracy of a QR as long as cond(J_b)^2 u < 1, which is also where the first
//                factorisation stops succeeding.  LDS: two chunk images over the place of G, Y, Y2 and 256 partial sums
//                (103.5 KB at nb = 64: one workgroup per CU; k_bd_cov's two matrices allow two).
//                A block whose factorisation fails gets NaN in its rows and in s2[b], its column in binfo[b].
//   then k_lev_diag with the per-block s2.
#include <algorithm>
#include <cmath>

#include "lsq_solver.h"
#include "lsq_cov.h"

constexpr int LV_T = 64;            // tile
constexpr int LV_KC = 32;           // k's staged per step
constexpr int LV_KS = LV_KC + 2;    // LDS row stride (doubles)
typedef double lv_v4d __attribute__((ext_vector_type(4)));

// wave and fragment layout of k_cov_xxt: four wavefronts own the 32 x 32 quadrants, 2 x 2 MFMA 16 x 16 x 4 tiles each; operand A:
// lane & 15 = row, lane >> 4 = k; operand B: lane & 15 = column; accumulator r: row (lane >> 4) + 4 r.
// A: p x n, column-major with leading dimension lda; column k of the product's left operand is A[:, jp[k]] (jp null: k) times
// scale[jp[k]] (scale null: 1).  X: n x n column-major, upper triangular, nothing below the diagonal is read.
__global__ void __launch_bounds__(256)
k_lev_tall(const double *__restrict__ A, int lda, int p, int n, const double *__restrict__ X, const int *__restrict__ jp,
           const double *__restrict__ scale, double *__restrict__ q) {
    __shared__ double sA[LV_T * LV_KS];
    __shared__ double sB[LV_T * LV_KS];
    __shared__ double sQ[2][LV_T];
    const int i0 = (int)blockIdx.x * LV_T;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wr = (w >> 1) * 32, wc = (w & 1) * 32;
    // staging of A: lane = row (coalesced down a column), 8 k's per thread; of X: lane & 31 = k (coalesced down a column of X),
    // 8 columns per thread
    const int am = tid & 63, akq = (tid >> 6) * 8;
    const int ia = i0 + am;
    const bool arow = ia < p;
    const int bk = tid & 31, bc = tid >> 5;
    double run[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) run[a][r] = 0.0;
    const int nt = (n + LV_T - 1) / LV_T;
    for (int tj = 0; tj < nt; ++tj) {
        const int j0 = tj * LV_T;
        const int kend = j0 + LV_T < n ? j0 + LV_T : n;      // k <= column < n
        lv_v4d acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) acc[a][b] = (lv_v4d){0.0, 0.0, 0.0, 0.0};
        double ra[8], rb[8];
        auto fetch = [&](int k0) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int k = k0 + akq + u;
                double v = 0.0;
                if (arow && k < kend) {
                    const int c = jp ? jp[k] : k;
                    v = A[(size_t)c * lda + ia];
                    if (scale) v = v * scale[c];
                }
                ra[u] = v;
            }
            const int k = k0 + bk;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int c = j0 + bc + 8 * u;
                rb[u] = (c < n && k <= c) ? X[(size_t)c * n + k] : 0.0;
            }
        };
        fetch(0);
        for (int k0 = 0; k0 < kend; k0 += LV_KC) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                sA[am * LV_KS + akq + u] = ra[u];
                sB[(bc + 8 * u) * LV_KS + bk] = rb[u];
            }
            __syncthreads();
            if (k0 + LV_KC < kend) fetch(k0 + LV_KC);
#pragma unroll
            for (int kk = 0; kk < LV_KC; kk += 4) {
                const int ko = kk + (lane >> 4);
                const double a0 = sA[(wr + (lane & 15)) * LV_KS + ko];
                const double a1 = sA[(wr + 16 + (lane & 15)) * LV_KS + ko];
                const double b0 = sB[(wc + (lane & 15)) * LV_KS + ko];
                const double b1 = sB[(wc + 16 + (lane & 15)) * LV_KS + ko];
                acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
            }
            __syncthreads();
        }
        // the squares of this tile's 2 x 16 columns of the lane, into the lane's row sums
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) run[a][r] = run[a][r] + (acc[a][0][r] * acc[a][0][r] + acc[a][1][r] * acc[a][1][r]);
    }
    // the 16 lanes of a row (a fixed butterfly), then the two wavefronts that hold the row's two column halves
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double v = run[a][r];
#pragma unroll
            for (int off = 8; off >= 1; off >>= 1) v += __shfl_xor(v, off);
            if ((lane & 15) == 0) sQ[w & 1][wr + a * 16 + (lane >> 4) + 4 * r] = v;
        }
    __syncthreads();
    if (tid < LV_T && i0 + tid < p) q[i0 + tid] = sQ[0][tid] + sQ[1][tid];
}

// (q, f, s2) -> se, t, cook; the order of the operations is the specification (include/lsqhip.h) and the numpy twin's.  s2b
// non-null: row i belongs to block i / mb and takes s2b[i / mb] (lsq_solver_leverage); else the one s2.  ncook: the number of
// parameters of the fit, as a double.  f is read only for t and cook.
__global__ void __launch_bounds__(256)
k_lev_diag(long long m, const double *__restrict__ q, const double *__restrict__ f, double s2, const double *__restrict__ s2b,
           int mb, double ncook, double *__restrict__ se, double *__restrict__ t, double *__restrict__ cook) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const double sd = sqrt(s2b ? s2b[i / mb] : s2);
    const double h = q[i];
    if (se) se[i] = sd * sqrt(h);
    if (t || cook) {
        const double d = 1.0 - h;
        const double ti = f[i] / (sd * sqrt(d));
        if (t) t[i] = ti;
        if (cook) cook[i] = ((ti * ti) * h) / (ncook * d);
    }
}

// ---------------------------------------------------------------------------------------------
// block-diagonal handle
// ---------------------------------------------------------------------------------------------
constexpr int BL_R = 32;           // rows per streamed chunk (k_bd_cov's)
constexpr int BL_CS = BL_R + 2;    // column stride of the staged chunk (doubles)
constexpr int BL_MISC = 8;         // doubles behind the matrices: [0] sum(f_b.^2), [1] (as ints) first failing column
constexpr int BL_HP = 256;         // partial row sums of the last pass: 32 rows x up to 8 threads per row

// doubles of LDS per block (= per group of G wavefronts): R0 (M, later the raw and the transformed chunk: two chunk images of
// ncp x BL_CS >= ncp x S64_LS) | W (Y) | W2 (Y2) | partial sums | misc
static inline size_t bl_group_doubles(int nb) {
    const size_t ncp = 16 * (size_t)((nb + 15) / 16);
    return ncp * 2 * BL_CS + 2 * ncp * S64_LS + BL_HP + BL_MISC;
}

template <int G>
__global__ void __launch_bounds__(256)
k_bd_lev(int B, int mb, int nb, const double *__restrict__ vals, const double *__restrict__ scale,
         const double *__restrict__ f, double *__restrict__ hout, double *__restrict__ s2out, int *__restrict__ binfo) {
    extern __shared__ double bl_lds[];
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
    const int csz = ncp * BL_CS;               // one chunk image
    double *M = bl_lds + (G == 4 ? 0 : wv) * (size_t)(2 * csz + 2 * msz + BL_HP + BL_MISC);
    double *W = M + 2 * csz;                   // chunk staging while streaming, then Y = inv(U)'
    double *W2 = W + msz;                      // Y2 = inv(U2)'
    double *ch = W;
    double *ach = M, *zch = M + csz;           // passes 2 and 3: the raw chunk and the chunk of z = Y a, over the place of M
    double *hp = W2 + msz;                     // pass 3: partial row sums
    double *misc_d = hp + BL_HP;               // [0] sum(f_b.^2)
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
    const int nch = (mb + BL_R - 1) / BL_R;
    load(0);
    for (int c = 0; c < nch; ++c) {
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int col = c0 + p * CP;
            if (col < ncp) ch[col * BL_CS + lr] = reg[p];      // (columns nb .. ncp-1: zeros)
        }
        ssq += freg * freg;                                    // (lanes 32 .. of the group: zeros)
        __syncthreads();
        if (c + 1 < nch) load((c + 1) * BL_R);                 // in flight during the tile products
#pragma unroll
        for (int ks = 0; ks < BL_R / 4; ++ks) {
            const int kk = 4 * ks + kq;
#pragma unroll
            for (int q = 0; q < TPW; ++q) {
                if (has[q]) {
                    const double a = ch[(16 * ti[q] + ij) * BL_CS + kk];
                    const double bb = ch[(16 * tj[q] + ij) * BL_CS + kk];
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

    // ---- M = U'U, unpivoted (the blocked scheme of k_bd_solve<.., false> on NT tile rows), then Wt = inv(U)' (block lower
    // triangular, zeros above the diagonal inside the diagonal tiles); ends behind a barrier ----
    auto factor_invert = [&](double *Wt) {
        for (int kb = 0; kb < NT; ++kb) {
            const int o = 16 * kb;
            if (wg == 0) {
                const int bad = s64_chol16(M, Wt, o, lane);
                if (bad && lane == 0 && misc_i[0] == 0) misc_i[0] = o + bad;
            }
            __syncthreads();
            const int nt = NT - 1 - kb;
            for (int q = wg; q < nt; q += G) {             // row panel: U[o.., t] = inv(U_kk)' G[o.., t]
                const int t = kb + 1 + q;
                s64_v4d a = {0.0, 0.0, 0.0, 0.0};
                s64_tile_mma<false, false>(a, Wt, o, o, M, o, 16 * t, 1, lane);
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
        cov_inv_levels<G>(M, Wt, NT, wg, lane);
        __syncthreads();
    };
    factor_invert(W);                          // G_b = U'U, Y = inv(U)'
    if (s2out && live && gt == 0 && !hout) {   // (the variances alone)
        s2out[b] = misc_i[0] ? NAN : misc_d[0] / (double)(mb - nb);
        if (binfo) binfo[b] = misc_i[0];
    }
    if (!hout) return;                         // (the same for every thread of the launch)

    // one chunk of 32 rows: the raw rows (column scale applied) into ach, then z = Y a into zch; thread (lr, c0) owns the
    // entries r = c0 + p CP of its row, k in index order.  Ends behind a barrier; the caller has one before the next call
    auto stage_z = [&](int c) {
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int col = c0 + p * CP;
            if (col < ncp) ach[col * BL_CS + lr] = scale ? reg[p] * sc(col) : reg[p];   // (columns nb .. ncp-1: zeros)
        }
        __syncthreads();
        if (c + 1 < nch) load((c + 1) * BL_R);
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int r = c0 + p * CP;
            if (r < ncp) {
                double z = 0.0;
                if (r < nb) {
                    const double *Yr = W + r * S64_LS;
                    for (int k = 0; k <= r; ++k) z = z + Yr[k] * ach[k * BL_CS + lr];
                }
                zch[r * BL_CS + lr] = z;
            }
        }
        __syncthreads();
    };

    // ---- second pass over J_b: G2 = sum z z' (the Gram matrix of Q1 = J_b inv(U): the identity up to cond(G_b) u) ----
#pragma unroll
    for (int q = 0; q < TPW; ++q) acc[q] = s64_v4d{0.0, 0.0, 0.0, 0.0};
    const double *fkeep = f;
    f = nullptr;                               // (load: the residual is not read again)
    load(0);
    for (int c = 0; c < nch; ++c) {
        stage_z(c);
#pragma unroll
        for (int ks = 0; ks < BL_R / 4; ++ks) {
            const int kk = 4 * ks + kq;
#pragma unroll
            for (int q = 0; q < TPW; ++q) {
                if (has[q]) {
                    const double a = zch[(16 * ti[q] + ij) * BL_CS + kk];
                    const double bb = zch[(16 * tj[q] + ij) * BL_CS + kk];
                    acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bb, acc[q], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
        if (has[q]) {
            const int j = 16 * tj[q] + ij;
#pragma unroll
            for (int r = 0; r < 4; ++r) M[(16 * ti[q] + kq + 4 * r) * S64_LS + j] = acc[q][r];
        }
    }
    __syncthreads();
    if (gt < ncp && (!live || gt >= nb)) M[gt * S64_LS + gt] = 1.0;    // padding: identity
    __syncthreads();
    factor_invert(W2);                         // G2 = U2'U2, Y2 = inv(U2)': J_b = (Q1 inv(U2)) (U2 U), CholeskyQR2
    const int fail = misc_i[0];
    double s2 = fkeep ? misc_d[0] / (double)(mb - nb) : 1.0;
    if (fail) s2 = NAN;
    if (live && gt == 0) {
        if (binfo) binfo[b] = fail;
        if (s2out) s2out[b] = s2;
    }

    // ---- third pass: h_i = ||Y2 z_i||^2, z_i = Y a_i; thread (lr, c0) adds the squares of its entries in index order, the
    // CP threads of a row are added in index order ----
    load(0);
    for (int c = 0; c < nch; ++c) {
        stage_z(c);
        double part = 0.0;
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int r = c0 + p * CP;
            if (r < nb) {
                const double *Yr = W2 + r * S64_LS;
                double w = 0.0;
                for (int k = 0; k <= r; ++k) w = w + Yr[k] * zch[k * BL_CS + lr];
                part = part + w * w;
            }
        }
        hp[c0 * 32 + lr] = part;
        __syncthreads();
        const int row = c * BL_R + lr;
        if (gt < 32 && live && row < mb) {
            double h = 0.0;
#pragma unroll
            for (int u = 0; u < CP; ++u) h = h + hp[u * 32 + lr];
            hout[fbase + row] = fail ? NAN : h;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
int lsq_lev_scratch(lsq_solver *s, size_t doubles, double **out) {
    if (s->lev_cap < doubles) {
        if (s->d_lev_buf) {
            LSQ_HIP(hipStreamSynchronize(s->ctx->stream));
            LSQ_HIP(hipFree(s->d_lev_buf));
            s->d_lev_buf = nullptr;
            s->lev_cap = 0;
        }
        LSQ_HIP(hipMalloc(&s->d_lev_buf, (doubles + 8) * sizeof(double)));
        s->lev_cap = doubles;
    }
    *out = s->d_lev_buf;
    return LSQ_OK;
}

extern "C" int lsq_dense_qr_leverage(lsq_solver *s, lsq_mat *J, const double *d_A, int p, int lda, const double *d_f,
                                     double *d_q, double *d_se, double *d_student, double *d_cook, double *h_s2, int *h_info) {
    LSQ_RANGE("lsq_dense_qr_leverage");
    if (!s || !J) { lsq_set_error("lsq_dense_qr_leverage: null argument"); return LSQ_EARG; }
    if (!d_q && !d_se && !d_student && !d_cook && !h_s2) {
        lsq_set_error("lsq_dense_qr_leverage: d_q, d_se, d_student, d_cook and h_s2 are all NULL: nothing to compute");
        return LSQ_EARG;
    }
    if (s->kind != LSQ_QR || !s->d_qr) {
        lsq_set_error("lsq_dense_qr_leverage: needs a QR() solver created on a dense Jacobian (lsq_dense_create); this "
                      "solver's kind is %d (a Cholesky() solver on a block-diagonal handle has lsq_solver_leverage)", s->kind);
        return LSQ_EARG;
    }
    if (J->kind != LSQ_MAT_DENSE) {
        lsq_set_error("lsq_dense_qr_leverage: the Jacobian is not a dense handle (lsq_dense_create); block-diagonal handles "
                      "have lsq_solver_leverage, bordered ones lsq_bordered_qr_leverage, CSC and operator handles are not offered");
        return LSQ_EARG;
    }
    if (J->m != s->m || J->n != s->n) {
        lsq_set_error("lsq_dense_qr_leverage: this solver was allocated for a %d x %d Jacobian, got %d x %d", s->m, s->n, J->m, J->n);
        return LSQ_EARG;
    }
    const int m = J->m, n = J->n;
    if (m < n) {
        lsq_set_error("lsq_dense_qr_leverage: inv(J'J) needs m >= n (got m = %d, n = %d)", m, n);
        return LSQ_EARG;
    }
    if (d_f && m <= n) {
        lsq_set_error("lsq_dense_qr_leverage: the residual variance sum(f.^2) / (m - n) needs m > n (got m = %d, n = %d); "
                      "pass d_f = NULL for the quadratic forms alone", m, n);
        return LSQ_EARG;
    }
    if (!d_f && (d_se || d_student || d_cook || h_s2)) {
        lsq_set_error("lsq_dense_qr_leverage: d_se, d_student, d_cook and h_s2 need the residual d_f (s^2 = sum(f.^2) / (m - n)); "
                      "without it only d_q is available");
        return LSQ_EARG;
    }
    if (d_A && (d_student || d_cook)) {
        lsq_set_error("lsq_dense_qr_leverage: d_student and d_cook belong to the rows of J itself (they pair q_i with f_i); "
                      "with new rows d_A they must be NULL");
        return LSQ_EARG;
    }
    if (d_A && (p < 1 || lda < p)) {
        lsq_set_error("lsq_dense_qr_leverage: d_A is p x n column-major and needs p >= 1 and lda >= p (got p = %d, lda = %d)", p, lda);
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
        lsq_set_error("RankDeficientException(%d): lsq_dense_qr_leverage: the Jacobian has rank %d < n = %d (xGELSY's decision at "
                      "rcond = n eps); a pseudo-inverse covariance is not offered", rank, rank, n);
        return LSQ_ERANK;
    }
    const double s2 = d_f ? ssq / (double)(m - n) : 1.0;
    if (h_s2) *h_s2 = s2;
    if (!d_q && !d_se && !d_student && !d_cook) return LSQ_OK;
    const int rows = d_A ? p : m;
    double *q = d_q;
    if (!q) LSQ_TRY(lsq_lev_scratch(s, (size_t)rows, &q));
    if (d_A) {
        LSQ_LAUNCH(k_lev_tall, dim3(lsq_div_up(rows, LV_T)), dim3(256), 0, c->stream, d_A, lda, rows, n, X, jp,
                   (const double *)nullptr, q);
    } else {
        LSQ_LAUNCH(k_lev_tall, dim3(lsq_div_up(rows, LV_T)), dim3(256), 0, c->stream, (const double *)J->d_dense, m, rows, n, X,
                   jp, J->d_colscale, q);
    }
    if (d_se || d_student || d_cook)
        LSQ_LAUNCH(k_lev_diag, dim3(lsq_div_up(rows, 256)), dim3(256), 0, c->stream, (long long)rows, (const double *)q, d_f, s2,
                   (const double *)nullptr, 1, (double)n, d_se, d_student, d_cook);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

template <int G>
static int bd_lev_launch(lsq_ctx *c, lsq_mat *J, const double *d_f, double *d_h, double *d_s2, int *d_binfo) {
    const int B = J->bd_blocks;
    const size_t lds = (G == 4 ? 1 : 4) * bl_group_doubles(J->bd_nb) * sizeof(double);
    LSQ_TRY(lsq_set_lds(c, (const void *)k_bd_lev<G>, lds));
    const int grid = G == 4 ? B : (B + 3) / 4;
    LSQ_LAUNCH((k_bd_lev<G>), dim3(grid), dim3(256), lds, c->stream, B, J->bd_mb, J->bd_nb, (const double *)J->csc.d_val,
               J->d_colscale, d_f, d_h, d_s2, d_binfo);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

extern "C" int lsq_solver_leverage(lsq_solver *s, lsq_mat *J, const double *d_f, double *d_h, double *d_se, double *d_student,
                                   double *d_cook, double *d_s2, int *h_info) {
    LSQ_RANGE("lsq_solver_leverage");
    if (!s || !J) { lsq_set_error("lsq_solver_leverage: null argument"); return LSQ_EARG; }
    if (!d_h && !d_se && !d_student && !d_cook && !d_s2) {
        lsq_set_error("lsq_solver_leverage: d_h, d_se, d_student, d_cook and d_s2 are all NULL: nothing to compute");
        return LSQ_EARG;
    }
    if (J->kind == LSQ_MAT_DENSE) {
        lsq_set_error("lsq_solver_leverage: the Jacobian is a dense handle; use lsq_dense_qr_leverage with a QR() solver on it");
        return LSQ_EARG;
    }
    if (J->kind == LSQ_MAT_OP) {
        lsq_set_error("lsq_solver_leverage: not offered on an operator handle (no stored values); leverages need a dense "
                      "(lsq_dense_qr_leverage) or block-diagonal handle");
        return LSQ_EARG;
    }
    if (J->br_blocks) {
        lsq_set_error("lsq_solver_leverage: not built for a bordered block-diagonal handle (the shared columns couple the blocks); "
                      "lsq_bordered_qr_leverage with a BorderedQR() solver gives the leverages there, lsq_solver_covariance or "
                      "lsq_bordered_qr_covariance the parameter covariance");
        return LSQ_EARG;
    }
    if (J->bd_blocks == 0) {
        lsq_set_error("lsq_solver_leverage: not offered on a general CSC handle; lsq_sparse_covariance gives the parameter "
                      "covariance there, a dense handle has lsq_dense_qr_leverage");
        return LSQ_EARG;
    }
    if (s->kind != LSQ_CHOLESKY || s->bd_blocks == 0) {
        lsq_set_error("lsq_solver_leverage: needs a Cholesky() solver created on a block-diagonal Jacobian (lsq_blockdiag_create); "
                      "this solver's kind is %d (a QR() solver on a dense handle has lsq_dense_qr_leverage)", s->kind);
        return LSQ_EARG;
    }
    if (J->bd_blocks != s->bd_blocks || J->bd_mb != s->bd_mb || J->bd_nb != s->bd_nb || J->m != s->m || J->n != s->n) {
        lsq_set_error("lsq_solver_leverage: this solver was allocated for a block-diagonal Jacobian of %d blocks of %d x %d",
                      s->bd_blocks, s->bd_mb, s->bd_nb);
        return LSQ_EARG;
    }
    const int B = s->bd_blocks, mb = s->bd_mb, nb = s->bd_nb;
    if (d_f && mb <= nb) {
        lsq_set_error("lsq_solver_leverage: the residual variance sum(f_b.^2) / (mb - nb) needs mb > nb (got mb = %d, nb = %d); "
                      "pass d_f = NULL for the leverages alone", mb, nb);
        return LSQ_EARG;
    }
    if (!d_f && (d_se || d_student || d_cook || d_s2)) {
        lsq_set_error("lsq_solver_leverage: d_se, d_student, d_cook and d_s2 need the residual d_f (s_b^2 = sum(f_b.^2) / (mb - nb)); "
                      "without it only d_h is available");
        return LSQ_EARG;
    }
    lsq_ctx *c = s->ctx;
    LSQ_HIP(hipSetDevice(c->device));
    LSQ_TRY(lsq_ensure_csc(J));        // (a device-side g! may have written the product mirrors only)
    if (!s->d_cov_info) LSQ_HIP(hipMalloc(&s->d_cov_info, (size_t)B * sizeof(int)));
    const bool derived = d_se || d_student || d_cook;
    const long long m = (long long)B * mb;
    double *h = d_h, *s2 = d_s2;
    if ((derived && (!h || !s2))) {
        double *buf = nullptr;
        LSQ_TRY(lsq_lev_scratch(s, (size_t)B + (size_t)m, &buf));
        if (!s2) s2 = buf;
        if (!h) h = buf + B;
    }
    if (nb > 16) LSQ_TRY(bd_lev_launch<4>(c, J, d_f, h, s2, s->d_cov_info));
    else LSQ_TRY(bd_lev_launch<1>(c, J, d_f, h, s2, s->d_cov_info));
    if (derived) {
        LSQ_LAUNCH(k_lev_diag, dim3(lsq_div_up(m, 256)), dim3(256), 0, c->stream, m, (const double *)h, d_f, 1.0, (const double *)s2,
                   mb, (double)nb, d_se, d_student, d_cook);
        LSQ_HIP(hipGetLastError());
    }
    if (h_info) {
        LSQ_HIP(hipMemcpyAsync(h_info, s->d_cov_info, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        LSQ_HIP(hipStreamSynchronize(c->stream));
    }
    return LSQ_OK;
}
