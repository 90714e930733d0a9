// Schur() on a bordered block-diagonal Jacobian J = [blkdiag(J_1 .. J_B) | C] (lsq_blockdiag_bordered_create) with nb <= 64 and
// ANY number ng of shared columns: LevenbergMarquardt's damped solve (J'J + D) x = J'y as right-looking unpivoted dpotrf on the
// stacked matrix with the locals first (dense_cholesky.jl:43-59), like Cholesky() on this handle (lsq_bordered.hip) -- but
// the border never has to fit one workgroup's LDS.  With U_bb'U_bb = J_b'J_b + D_b:
//     W_b = inv(U_bb)' J_b'C_b (nb x ng)        z_b = inv(U_bb)' J_b'y_b
//     S   = C'C + D_g - W'W                     r_g = C'y - W'z            (W: the (B nb) x ng stack of the W_b)
//     x_g = S \ r_g                             x_b = inv(U_bb) (z_b - W_b x_g)
// W_b is the block's rows U_bg of the stacked factor and S what dpotrf has left in the corner when it gets there, so the
// PosDefException column is b nb + k in a local block and B nb + k in the factor of S, the lowest one wins.  Nothing of size
// B ng^2 is written: the corner is two tall products on the dense path's SYRK kernel.  Stream order, one read of the status
// words per solve:
//   k_sc_eliminate   per block, the geometry of k_bd_solve on J_b alone (one workgroup per block; nb <= 16: one wavefront
//                    per block, four per workgroup): G_bb + D_b and J_b'y_b (fp64 MFMA upper tiles, y_b as one more operand
//                    column), in-LDS unpivoted Cholesky, forward solve -> U_b, z_b.  Then the border in tiles of 64 columns:
//                    P = J_b'C_b[:, tile] over the block's mb rows (row chunks in order; a wavefront keeps its 16 x 16 tiles
//                    of P in registers), W = inv(U_bb)'P by 16-row blocks (inv(U_kk)' P_k, then P_i -= U_ki' W_k: the
//                    accumulator registers are the MFMA's B operand, no trip through LDS), transposed through LDS and stored
//                    down the columns of the W stack.  LDS does not depend on ng.
//   lsq_syrk_partials  twice (k_syrk_mfma, lsq_dense_mfma.hip, unchanged): split-K partials of C'C with C'y riding along (C =
//                    the last ng columns of the CSC values, lda = m) and of W'W with W'z (lda = B nb).
//   k_sc_reduce      S = sum partials(C) - sum partials(W) + D_g into the inner solver's d_chol, r_g likewise; slices in
//                    index order, C before W; clears the inner solver's status word.
//   inner solver     a dense LSQ_CHOLESKY lsq_solver with n = ng owned by this one (lsq_solver::inner): the blocked
//                    factorisation and its triangular solves (lsq_cholesky_blocked_factor), or the one-workgroup dpotf2
//                    (lsq_cholesky_small_factor_ready) + k_sc_small_solve where lsq_cholesky_takes_blocked says no.
//   k_sc_back        one workgroup per block: x_b = inv(U_bb) (z_b - W_b x_g).
// No floating-point atomics, no workgroup waits for another outside the inner solver's one-launch factorisation, every sum
// has a fixed association: two runs give identical bits.  If that factorisation gives up on a bounded wait, S is formed again
// (k_sc_reduce) and factored by panel launches, once; the elimination is not repeated.
//
// Dogleg(Schur()) is not offered, for the reason lsq_bordered.hip gives for Dogleg(Cholesky()).
#include <climits>

#include "lsq_solver.h"
#include "lsq_small64.h"

int lsq_bordered_refuse_dogleg();                                                       // lsq_bordered.hip
int lsq_cholesky_blocked_factor(lsq_solver *s, int n, double *d_x, bool allow_tiles);   // lsq_dense_mfma.hip
int lsq_cholesky_blocked_solve(lsq_solver *s, int n, double *d_x);                      // lsq_dense_mfma.hip
int lsq_syrk_slices(const lsq_ctx *c, int krows, int ncols);                            // lsq_dense_mfma.hip
size_t lsq_syrk_partial_elems(int ncols, int kslices);                                  // lsq_dense_mfma.hip
int lsq_syrk_partials(lsq_ctx *c, const double *A, int lda, int krows, int ncols, int kslices, double *W, const double *jy,
                      double *jx);                                                      // lsq_dense_mfma.hip
const int *lsq_tri_pipe_err_ptr(lsq_solver *s);                                         // lsq_qr.hip
void lsq_tri_pipe_disable(lsq_solver *s);                                               // lsq_qr.hip

constexpr int SC_R = 32;           // rows per streamed chunk
constexpr int SC_CS = SC_R + 2;    // column stride of the staged chunk (doubles)
constexpr int SC_MISC = 104;       // y chunk (32) | right-hand side (64) | scalars (8)
constexpr int SC_TW = 64;          // border columns per tile
constexpr int SC_MT = 64;          // tile of the SYRK partials (lsq_dense_mfma.hip: MT)

// doubles of LDS per block (= per group of G wavefronts): M | W (G = 1: inside M) | misc | staged chunk of [J_b C_b[:, tile]]
static inline size_t sc_group_doubles(int nb, int G) {
    const size_t nbp = 16 * (size_t)((nb + 15) / 16);
    return (G == 4 ? 2 : 1) * nbp * S64_LS + SC_MISC + (nbp + SC_TW) * SC_CS;
}

__global__ void k_sc_init(int *info) {
    if (threadIdx.x == 0) { info[0] = INT_MAX; info[1] = INT_MAX; info[2] = 0; info[3] = 0; }
}

template <int G>
__global__ void __launch_bounds__(256)
k_sc_eliminate(int B, int mb, int nb, int ng, const double *__restrict__ vals, const double *__restrict__ scale,
               const double *__restrict__ y, const double *__restrict__ damp, double *__restrict__ Uout,
               double *__restrict__ zout, double *__restrict__ Wout, int *__restrict__ info) {
    extern __shared__ double sc_lds[];
    constexpr int GT = 64 * G;                 // threads per block of the matrix
    constexpr int TPW = G == 4 ? 3 : 1;        // upper tiles of G_bb per wavefront
    constexpr int CP = GT / 32;                // columns per load pass
    constexpr int NC = SC_TW / CP;             // load passes over one border tile
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wg = G == 4 ? __builtin_amdgcn_readfirstlane(wv) : 0;      // wavefront inside its group
    const int gt = G == 4 ? tid : lane;                                  // thread inside its group
    const int b = G == 4 ? (int)blockIdx.x : (int)blockIdx.x * 4 + wv;
    const bool live = b < B;
    const int NT = (nb + 15) >> 4, nbp = 16 * NT;
    const int msz = nbp * S64_LS;
    double *M = sc_lds + (G == 4 ? 0 : wv) * ((G == 4 ? 2 : 1) * (size_t)msz + SC_MISC + (size_t)(nbp + SC_TW) * SC_CS);
    double *W = G == 4 ? M + msz : M + 16;     // inv(U_kk)' (G = 1: one 16 x 16 block, in the unused columns 16 .. 31 of M)
    double *ych = M + (G == 4 ? 2 : 1) * msz;
    double *rv = ych + 32;
    int *misc_i = (int *)(rv + 64 + 1);        // [1] first failing local column
    double *ch = rv + 64 + 8;                  // staged chunk of J_b: [column][row]
    double *cc = ch + nbp * SC_CS;             // ... and of the border tile
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
    const bool rtile = wg < NT;                // this wavefront forms rows 16 wg .. of r = J_b'y_b

    // ---- stream J_b: G_bb (upper tiles) and r_b ----
    const size_t m = (size_t)B * mb;
    const size_t vbase = live ? (size_t)b * mb * nb : 0;
    const size_t cbase = m * nb + (live ? (size_t)b * mb : 0);
    const size_t ybase = live ? (size_t)b * mb : 0;
    const int lr = gt & 31, c0 = gt >> 5;
    double reg[8], yreg = 0.0;
    auto load = [&](int row0) {
        const int row = row0 + lr;
        const bool ok = live && row < mb;
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int c = c0 + p * CP;
            reg[p] = (ok && c < nb) ? vals[vbase + (size_t)c * mb + row] : 0.0;
        }
        if (gt < 32) yreg = ok ? y[ybase + row] : 0.0;
    };
    const int nch = (mb + SC_R - 1) / SC_R;
    {
        s64_v4d acc[TPW], racc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < TPW; ++q) acc[q] = s64_v4d{0.0, 0.0, 0.0, 0.0};
        load(0);
        for (int c = 0; c < nch; ++c) {
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const int col = c0 + p * CP;
                if (col < nbp) ch[col * SC_CS + lr] = reg[p];      // (columns nb .. nbp-1: zeros)
            }
            if (gt < 32) ych[gt] = yreg;
            __syncthreads();
            if (c + 1 < nch) load((c + 1) * SC_R);                 // in flight during the tile products
#pragma unroll
            for (int ks = 0; ks < SC_R / 4; ++ks) {
                const int kk = 4 * ks + kq;
#pragma unroll
                for (int q = 0; q < TPW; ++q) {
                    if (has[q]) {
                        const double a = ch[(16 * ti[q] + ij) * SC_CS + kk];
                        const double bb = ch[(16 * tj[q] + ij) * SC_CS + kk];
                        acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bb, acc[q], 0, 0, 0);
                    }
                }
                if (rtile) {
                    const double a = ch[(16 * wg + ij) * SC_CS + kk];
                    const double bb = ij == 0 ? ych[kk] : 0.0;
                    racc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bb, racc, 0, 0, 0);
                }
            }
            __syncthreads();
        }
        // ---- G_bb (column-scaled handle: S_b G_V S_b, r = S_b r_V) into M, r into rv ----
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
        if (rtile && ij == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 16 * wg + kq + 4 * r;
                rv[i] = racc[r] * sc(i);
            }
        }
    }
    if (gt == 0) misc_i[1] = 0;
    __syncthreads();
    if (gt < nbp) {
        if (!live || gt >= nb) M[gt * S64_LS + gt] = 1.0;                          // padding: identity
        else M[gt * S64_LS + gt] += damp[(size_t)b * nb + gt];
    }
    __syncthreads();

    // ---- dense_cholesky.jl:43-59 on the block: G_bb + D_b = U_bb'U_bb, unpivoted (the blocked scheme of s64_chol on NT tile rows) ----
    for (int kb = 0; kb < NT; ++kb) {
        const int o = 16 * kb;
        if (wg == 0) {
            const int bad = s64_chol16(M, W, o, lane);
            if (bad && lane == 0 && misc_i[1] == 0) misc_i[1] = o + bad;
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
    // a block that failed goes on as padding would (the wavefronts of a workgroup share the barriers below) and stores zeros:
    // what follows it in the stream works on finite numbers, and the solve reports this block's column whatever they give
    const int fail = misc_i[1];
    if (fail && live && gt == 0) {
        atomicMin(&info[0], b * nb + fail);
        atomicMin(&info[1], b);
    }
    if (wg == 0) {
        // U_bb'z = r_b: one wavefront, lane = unknown, the pivot row broadcast with v_readlane
        const bool in = lane < nbp;
        const int li = in ? lane : 0;
        const double dinv = 1.0 / M[li * S64_LS + li];
        double z = in ? rv[li] : 0.0;
#pragma unroll 4
        for (int k = 0; k < nbp; ++k) {
            const double u = M[k * S64_LS + li];
            const double zk = s64_readlane(z * dinv, k);
            if (lane == k) z = zk;
            else if (in && lane > k) z -= u * zk;
        }
        if (live && lane < nb) zout[(size_t)b * nb + lane] = fail ? 0.0 : z;
    }
    if (live) {
        double *ub = Uout + (size_t)b * nb * nb;
        for (int e = gt; e < nb * nb; e += GT) {       // rows of U_bb, zeros below the diagonal
            const int k = e / nb, c = e - k * nb;
            ub[e] = c >= k ? M[k * S64_LS + c] : 0.0;
        }
    }

    // ---- the border, 64 columns at a time: P = J_b'C_b[:, tile], W = inv(U_bb)'P ----
    // G = 4: wavefront wg holds the NT tile rows of tile column wg;  G = 1: the wavefront holds the four tile columns of its
    // one tile row.  pt[q]: D layout of the MFMA, entry [row (lane >> 4) + 4 r][column lane & 15] in register r.
    const size_t ldw = (size_t)B * nb;
    const int tls = nbp + 1;                           // stride of the transposed tile [column][row] in the staging area
    double creg[NC];
    auto load_border = [&](int row0, int col0) {
        const int row = row0 + lr;
        const bool ok = live && row < mb;
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int c = c0 + p * CP;
            reg[p] = (ok && c < nb) ? vals[vbase + (size_t)c * mb + row] : 0.0;
        }
#pragma unroll
        for (int p = 0; p < NC; ++p) {
            const int c = col0 + c0 + p * CP;
            creg[p] = (ok && c < ng) ? vals[cbase + (size_t)c * m + row] : 0.0;
        }
    };
    const int ntile = (ng + SC_TW - 1) / SC_TW;
    for (int t = 0; t < ntile; ++t) {
        const int col0 = SC_TW * t;
        s64_v4d pt[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) pt[q] = s64_v4d{0.0, 0.0, 0.0, 0.0};
        load_border(0, col0);
        for (int c = 0; c < nch; ++c) {
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const int col = c0 + p * CP;
                if (col < nbp) ch[col * SC_CS + lr] = reg[p];
            }
#pragma unroll
            for (int p = 0; p < NC; ++p) cc[(c0 + p * CP) * SC_CS + lr] = creg[p];
            __syncthreads();
            if (c + 1 < nch) load_border((c + 1) * SC_R, col0);
#pragma unroll
            for (int ks = 0; ks < SC_R / 4; ++ks) {
                const int kk = 4 * ks + kq;
                if (G == 4) {
                    const double bb = cc[(16 * wg + ij) * SC_CS + kk];
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (q < NT) pt[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(ch[(16 * q + ij) * SC_CS + kk], bb, pt[q], 0, 0, 0);
                } else {
                    const double a = ch[ij * SC_CS + kk];
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        pt[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, cc[(16 * q + ij) * SC_CS + kk], pt[q], 0, 0, 0);
                }
            }
            __syncthreads();
        }
        if (scale) {                                   // S_b P_V S_g
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = col0 + (G == 4 ? 16 * wg : 16 * q) + ij;
                const double sj = (live && j < ng) ? scale[ldw + j] : 1.0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = (G == 4 ? 16 * q : 0) + kq + 4 * r;
                    const double si = (live && i < nb) ? scale[(size_t)b * nb + i] : 1.0;
                    pt[q][r] = pt[q][r] * (si * sj);
                }
            }
        }
        // forward substitution by 16-row blocks, what the row panel and the trailing update of the factorisation do to the
        // border columns of the stacked matrix.  The k index of a product runs over (lane >> 4) + 4 r in step r, so that the
        // registers of a D tile are its B operand as they stand.
        if (G == 4) {
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) {
                if (kb < NT) {
                    const int o = 16 * kb;
                    s64_v4d w = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        w = __builtin_amdgcn_mfma_f64_16x16x4f64(W[(o + ij) * S64_LS + o + kq + 4 * r], pt[kb][r], w, 0, 0, 0);
                    pt[kb] = w;
#pragma unroll
                    for (int i = kb + 1; i < 4; ++i) {
                        if (i < NT) {
                            s64_v4d u = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                u = __builtin_amdgcn_mfma_f64_16x16x4f64(M[(o + kq + 4 * r) * S64_LS + 16 * i + ij], w[r], u, 0, 0, 0);
                            pt[i] = pt[i] - u;
                        }
                    }
                }
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                s64_v4d w = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    w = __builtin_amdgcn_mfma_f64_16x16x4f64(W[ij * S64_LS + kq + 4 * r], pt[q][r], w, 0, 0, 0);
                pt[q] = w;
            }
        }
        // transposed into the staging area (free since the last barrier), then down the columns of the W stack
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (G == 1 || q < NT) {
                const int j = (G == 4 ? 16 * wg : 16 * q) + ij;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = (G == 4 ? 16 * q : 0) + kq + 4 * r;
                    ch[j * tls + i] = pt[q][r];
                }
            }
        }
        __syncthreads();
        if (live) {
            const int ncol = ng - col0 < SC_TW ? ng - col0 : SC_TW;
            for (int e = gt; e < ncol * nb; e += GT) {
                const int j = e / nb, i = e - j * nb;
                Wout[(size_t)(col0 + j) * ldw + (size_t)b * nb + i] = fail ? 0.0 : ch[j * tls + i];
            }
        }
        __syncthreads();
    }
}

// S (upper triangle, column-major, ld ng) = sum of the ksc partials of C'C - sum of the ksw partials of W'W + D_g, slices in
// index order, one thread per entry; column-scaled handle: the C sum times s_i s_j (W carries its factors already).  The
// workgroups behind the tiles: r_g = s .* (C'y) - W'z into rg (kept for a repeated solve) and xg (solved in place).
__global__ void __launch_bounds__(256)
k_sc_reduce(const double *__restrict__ PC, int ksc, const double *__restrict__ PW, int ksw, int ng,
            const double *__restrict__ cy, const double *__restrict__ wz, const double *__restrict__ sg,
            const double *__restrict__ damp_g, double *__restrict__ S, double *__restrict__ rg, double *__restrict__ xg,
            int *__restrict__ inner_info) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *inner_info = 0;   // the inner factorisation's status word, as k_syrk_reduce clears it
    const int nt = (ng + SC_MT - 1) / SC_MT;
    const int ntiles = nt * (nt + 1) / 2;
    if ((int)blockIdx.x >= ntiles * 16) {
        const int i = ((int)blockIdx.x - ntiles * 16) * 256 + threadIdx.x;
        if (i < ng) {
            const double c = sg ? cy[i] * sg[i] : cy[i];
            const double v = c - wz[i];
            rg[i] = v;
            xg[i] = v;
        }
        return;
    }
    const int tile = blockIdx.x / 16, part = blockIdx.x % 16;   // 16 workgroups per tile, 256 entries each
    int t = tile, bi = 0;
    while (t >= nt - bi) { t -= nt - bi; ++bi; }
    const int bj = bi + t;
    const int e = part * 256 + threadIdx.x;
    const int row = e % SC_MT, col = e / SC_MT;
    const int gi = bi * SC_MT + row, gj = bj * SC_MT + col;
    if (gi < ng && gj < ng && gi <= gj) {
        double c = 0.0, w = 0.0;
        for (int sl = 0; sl < ksc; ++sl) c += PC[((size_t)sl * ntiles + tile) * (SC_MT * SC_MT) + e];
        for (int sl = 0; sl < ksw; ++sl) w += PW[((size_t)sl * ntiles + tile) * (SC_MT * SC_MT) + e];
        if (sg) c = c * (sg[gi] * sg[gj]);
        double s = c - w;
        if (gi == gj) s += damp_g[gi];
        S[(size_t)gj * ng + gi] = s;
    }
}

// U'z = b, U x = z on the factor the one-workgroup dpotf2 left in U (upper, column-major, ld n; n < 64): one wavefront, lane =
// unknown.  Nothing is done when the factorisation stopped (*info != 0).
__global__ void __launch_bounds__(64)
k_sc_small_solve(const double *__restrict__ U, int n, double *__restrict__ bx, const int *__restrict__ info) {
    if (*info != 0) return;
    const int lane = threadIdx.x;
    const bool in = lane < n;
    const int li = in ? lane : 0;
    const double dinv = 1.0 / U[(size_t)li * n + li];
    double z = in ? bx[li] : 0.0;
    for (int k = 0; k < n; ++k) {
        const double u = U[(size_t)li * n + k];        // U[k, lane]
        const double zk = s64_readlane(z * dinv, k);
        if (lane == k) z = zk;
        else if (in && lane > k) z -= u * zk;
    }
    for (int k = n - 1; k >= 0; --k) {
        const double u = U[(size_t)k * n + li];        // U[lane, k]
        const double xk = s64_readlane(z * dinv, k);
        if (lane == k) z = xk;
        else if (lane < k) z -= u * xk;
    }
    if (in) bx[lane] = z;
}

// x_b = inv(U_bb) (z_b - W_b x_g): one workgroup per block.  The product W_b x_g: thread = (row i, column class jj), the thread
// sums the columns j = jj, jj + cpl, .. (cpl = 256 / nb classes) in ascending order; the first wavefront subtracts the classes
// in index order and substitutes back.
__global__ void __launch_bounds__(256)
k_sc_back(int B, int nb, int ng, const double *__restrict__ Uin, const double *__restrict__ zin, const double *__restrict__ Wst,
          const double *__restrict__ xg, double *__restrict__ x) {
    extern __shared__ double sc_lds[];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int ld = nb | 1;
    double *sU = sc_lds;
    double *sp = sU + nb * ld;                         // 256
    const double *ub = Uin + (size_t)b * nb * nb;
    for (int e = tid; e < nb * nb; e += 256) {
        const int k = e / nb, c = e - k * nb;
        sU[k * ld + c] = ub[e];
    }
    const size_t ldw = (size_t)B * nb;
    const int cpl = 256 / nb, i = tid % nb, jj = tid / nb;
    double p = 0.0;
    if (jj < cpl) {
        const double *wr = Wst + (size_t)b * nb + i;
        for (int j = jj; j < ng; j += cpl) p += wr[(size_t)j * ldw] * xg[j];
    }
    sp[tid] = p;
    __syncthreads();
    if (tid >= 64) return;
    const bool in = lane < nb;
    const int li = in ? lane : 0;
    double t = in ? zin[(size_t)b * nb + li] : 0.0;
    for (int q = 0; q < cpl; ++q) t -= sp[q * nb + li];
    const double dinv = 1.0 / sU[li * ld + li];
    for (int k = nb - 1; k >= 0; --k) {
        const double u = sU[li * ld + k];
        const double xk = s64_readlane(t * dinv, k);
        if (lane == k) t = xk;
        else if (lane < k) t -= u * xk;
    }
    if (in) x[(size_t)b * nb + lane] = t;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
struct ScLayout {
    int ksc, ksw;
    size_t U, z, W, cy, wz, rg, PC, PW, total;     // offsets into d_work (doubles)
};
static ScLayout sc_layout(const lsq_ctx *c, int B, int mb, int nb, int ng) {
    ScLayout l;
    l.ksc = lsq_syrk_slices(c, B * mb, ng);
    l.ksw = lsq_syrk_slices(c, B * nb, ng);
    const size_t Bn = (size_t)B * nb;
    l.U = 0;
    l.z = l.U + Bn * nb;
    l.W = l.z + Bn;
    l.cy = l.W + Bn * ng;
    l.wz = l.cy + ng;
    l.rg = l.wz + ng;
    l.PC = l.rg + ng;
    l.PW = l.PC + lsq_syrk_partial_elems(ng, l.ksc);
    l.total = l.PW + lsq_syrk_partial_elems(ng, l.ksw);
    return l;
}

int lsq_schur_solver_alloc(lsq_solver *s, const lsq_mat *J) {
    if (J->kind != LSQ_MAT_CSC || J->br_blocks < 1) {
        const char *what = J->kind == LSQ_MAT_DENSE ? "a dense handle (lsq_dense_create): use Cholesky() or QR()"
                           : J->kind != LSQ_MAT_CSC ? "an operator handle (lsq_op_create): use LSMR()"
                           : J->bd_blocks > 0       ? "a block-diagonal handle without shared columns (lsq_blockdiag_create): "
                                                      "use Cholesky() or BlockQR()"
                                                    : "a plain CSC handle (lsq_csc_create): use LSMR()";
        lsq_set_error("Schur() needs a bordered block-diagonal Jacobian (lsq_blockdiag_bordered_create); this is %s", what);
        return LSQ_EARG;
    }
    if (J->br_nb > 64) {
        lsq_set_error("Schur() on a bordered block-diagonal Jacobian needs nb <= 64 (got nb = %d, ng = %d): one block's normal "
                      "matrix must fit the 64 x 64 in-LDS factorisation. Use LSMR()", J->br_nb, J->br_ng);
        return LSQ_EARG;
    }
    if (!s->for_lm) return lsq_bordered_refuse_dogleg();
    lsq_ctx *c = s->ctx;
    s->br_blocks = J->br_blocks;
    s->br_mb = J->br_mb;
    s->br_nb = J->br_nb;
    s->br_ng = J->br_ng;
    const ScLayout l = sc_layout(c, J->br_blocks, J->br_mb, J->br_nb, J->br_ng);
    s->work_elems = l.total;
    LSQ_HIP(hipMalloc(&s->d_work, s->work_elems * sizeof(double)));
    LSQ_HIP(hipMalloc(&s->d_info, 4 * sizeof(int)));
    lsq_solver *in = new lsq_solver();     // the dense Cholesky() solver of the Schur complement: ng^2 doubles
    in->ctx = c;
    in->kind = LSQ_CHOLESKY;
    in->for_lm = 1;
    in->m = J->m;
    in->n = J->br_ng;
    const int st = lsq_dense_solver_alloc(in);
    if (st != LSQ_OK) {                    // (lsq_solver_create deletes s and nothing else)
        lsq_dense_solver_free(in);
        delete in;
        hipFree(s->d_work);
        hipFree(s->d_info);
        return st;
    }
    s->inner = in;
    return LSQ_OK;
}

template <int G>
static int sc_eliminate(lsq_ctx *c, lsq_solver *s, lsq_mat *J, const double *d_y, const double *d_damp, double *U, double *z,
                        double *W) {
    const int B = s->br_blocks;
    const size_t lds = (G == 4 ? 1 : 4) * sc_group_doubles(s->br_nb, G) * sizeof(double);
    LSQ_TRY(lsq_set_lds(c, (const void *)k_sc_eliminate<G>, lds));
    const int grid = G == 4 ? B : (B + 3) / 4;
    LSQ_LAUNCH((k_sc_eliminate<G>), dim3(grid), dim3(256), lds, c->stream, B, s->br_mb, s->br_nb, s->br_ng,
               (const double *)J->csc.d_val, J->d_colscale, d_y, d_damp, U, z, W, s->d_info);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

// dense_cholesky.jl:43-59 (damped, unpivoted, LM) on the stacked system
int lsq_schur_solve(lsq_solver *s, lsq_mat *J, const double *d_y, const double *d_damp, double *d_x, int *nmul) {
    lsq_ctx *c = s->ctx;
    if (!d_damp) return lsq_bordered_refuse_dogleg();
    if (J->kind != LSQ_MAT_CSC || J->br_blocks != s->br_blocks || J->br_mb != s->br_mb || J->br_nb != s->br_nb ||
        J->br_ng != s->br_ng || J->m != s->m || J->n != s->n) {
        lsq_set_error("Schur(): this solver was allocated for a bordered block-diagonal Jacobian of %d blocks of %d x %d with %d "
                      "shared columns; create a solver on the handle it is to solve with", s->br_blocks, s->br_mb, s->br_nb,
                      s->br_ng);
        return LSQ_EARG;
    }
    LSQ_HIP(hipSetDevice(c->device));
    LSQ_TRY(lsq_ensure_csc(J));        // (a device-side g! may have written the product mirrors only)
    const int B = s->br_blocks, mb = s->br_mb, nb = s->br_nb, ng = s->br_ng;
    const ScLayout l = sc_layout(c, B, mb, nb, ng);
    double *wk = s->d_work;
    double *U = wk + l.U, *z = wk + l.z, *W = wk + l.W, *cy = wk + l.cy, *wz = wk + l.wz, *rg = wk + l.rg;
    double *PC = wk + l.PC, *PW = wk + l.PW;
    double *xg = d_x + (size_t)B * nb;
    lsq_solver *in = s->inner;
    LSQ_LAUNCH(k_sc_init, dim3(1), dim3(64), 0, c->stream, s->d_info);
    if (nb > 16) LSQ_TRY(sc_eliminate<4>(c, s, J, d_y, d_damp, U, z, W));
    else LSQ_TRY(sc_eliminate<1>(c, s, J, d_y, d_damp, U, z, W));
    const double *C = (const double *)J->csc.d_val + (size_t)s->m * nb;    // the border: ng columns of m doubles
    LSQ_TRY(lsq_syrk_partials(c, C, s->m, s->m, ng, l.ksc, PC, d_y, cy));
    LSQ_TRY(lsq_syrk_partials(c, W, B * nb, B * nb, ng, l.ksw, PW, z, wz));
    const int nt = (ng + SC_MT - 1) / SC_MT, ntiles = nt * (nt + 1) / 2;
    const double *sg = J->d_colscale ? J->d_colscale + (size_t)B * nb : nullptr;
    const bool blocked = lsq_cholesky_takes_blocked(s->m, ng);
    const size_t lds_back = ((size_t)nb * (nb | 1) + 256) * sizeof(double);
    auto back = [&]() {
        LSQ_LAUNCH(k_sc_back, dim3(B), dim3(256), lds_back, c->stream, B, nb, ng, (const double *)U, (const double *)z,
                   (const double *)W, (const double *)xg, d_x);
        LSQ_HIP(hipGetLastError());
        return LSQ_OK;
    };
    int st4[4] = {0, 0, 0, 0};
    for (int attempt = 0; attempt < 2; ++attempt) {
        // (the factorisation overwrites d_chol: S is formed again for the retry, from the partials that still stand)
        LSQ_LAUNCH(k_sc_reduce, dim3(ntiles * 16 + lsq_div_up(ng, 256)), dim3(256), 0, c->stream, (const double *)PC, l.ksc,
                   (const double *)PW, l.ksw, ng, (const double *)cy, (const double *)wz, sg, d_damp + (size_t)B * nb,
                   in->d_chol, rg, xg, in->d_info);
        if (blocked) {
            LSQ_TRY(lsq_cholesky_blocked_factor(in, ng, xg, attempt == 0));
            in->last_chol_path = in->last_chol_tiles ? 4 : 2;
        } else {
            LSQ_TRY(lsq_cholesky_small_factor_ready(in, ng));
            LSQ_LAUNCH(k_sc_small_solve, dim3(1), dim3(64), 0, c->stream, (const double *)in->d_chol, ng, xg,
                       (const int *)in->d_info);
            in->last_chol_path = 1;
        }
        LSQ_TRY(back());
        // the one wait of the solve: the locals' verdict, the inner factorisation's, the solve pipeline's flag
        LSQ_TRY(lsq_read_ints(c, s->d_info, s->d_info + 1, in->d_info, blocked ? lsq_tri_pipe_err_ptr(in) : nullptr, st4));
        if (st4[2] != -1 || in->fb_tiles.off()) break;
        in->fb_tiles.gave_up(c, LSQ_FB_CHOL_TILES);    // the one-launch factorisation gave up on a wait: panel launches, once more
    }
    in->fb_tiles.solve_done(in->last_chol_path == 4);
    if (st4[3]) lsq_tri_pipe_disable(in);              // a wait of the pipelined triangular solves gave up
    else in->fb_pipe.solve_done(blocked && in->tripipe != nullptr);
    s->last_bd_path = 5;
    s->last_bd_block = -1;
    if (nmul) *nmul = 1;
    int col = 0;
    if (st4[1] != INT_MAX) {
        s->last_bd_block = st4[1];
        col = st4[0];
    } else if (st4[2] != 0) {
        s->last_bd_block = B;
        col = st4[2] > 0 ? B * nb + st4[2] : st4[2];
    }
    if (col != 0) {
        lsq_set_error("PosDefException: matrix is not positive definite; Cholesky failed at %d", col);
        return LSQ_ENOTPD;
    }
    if (st4[3]) {                      // (the factor is intact: only the two solves and the back substitution are repeated)
        LSQ_HIP(hipMemcpyAsync(xg, rg, (size_t)ng * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        LSQ_TRY(lsq_cholesky_blocked_solve(in, ng, xg));
        LSQ_TRY(back());
    }
    return LSQ_OK;
}
