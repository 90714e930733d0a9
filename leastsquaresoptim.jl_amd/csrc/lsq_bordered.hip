// Bordered block-diagonal Jacobians J = [blkdiag(J_1 .. J_B) | C]: J_b dense mb x nb (the local parameters of data set b),
// C dense (B*mb) x ng (the parameters shared by all data sets), nb + ng <= 64: the handle (lsq_blockdiag_bordered_create: a
// CSC handle that also knows its shape) and LevenbergMarquardt's Cholesky() on it.
//
// J'J + D is an arrowhead: B diagonal blocks J_b'J_b + D_b, a border J_b'C_b and the corner C'C + D_g.  With the locals
// ordered first the Cholesky factor has no fill, and right-looking dpotrf on the stacked matrix (dense_cholesky.jl:43-59)
// is: eliminate the locals block by block -- block b updates nothing but its own border rows and the corner, where its
// update is -U_bg'U_bg -- then factor what the corner has become, the Schur complement
//     S = D_g + sum_b (C_b'C_b - U_bg'U_bg).
// So the reference's semantics carry over exactly: one trust region, PosDefException at the 1-based column at which the
// stacked factorisation stops (a local column b*nb + k, or B*nb + k inside the Schur factor; the lowest one wins).  Three
// stream-ordered steps, no workgroup waits for another, the only word shared inside a launch is an integer atomicMin:
//   k_bb_eliminate  per block, the geometry of k_bd_solve on the AUGMENTED block A_b = [J_b C_b] (nb + ng <= 64 columns):
//                   one pass over the block's values and its mb rows of the border forms G = A_b'A_b + diag(damp_b, 0) and
//                   r = A_b'y_b (fp64 MFMA upper tiles, y_b as one more operand column); unpivoted Cholesky of the first nb
//                   columns ONLY; the forward solve of those nb columns.  What is left in the trailing ng x ng corner and in
//                   the trailing ng entries of the right-hand side is the block's Schur contribution.  Written per block:
//                   U_b (nb rows of nb + ng), z_b (nb), the contribution (upper triangle by rows, then the ng entries of
//                   the right-hand side).
//   k_bb_reduce     (B > BB_GS only) sums the contributions of BB_GS consecutive blocks, in index order, one thread per entry
//   k_bb_schur      one workgroup: sums the B contributions (or the partial sums) in index order, adds the border's damping,
//                   factors the ng x ng system in LDS, two triangular solves, writes x[B*nb ..]
//   k_bb_back       one wavefront per block: x_b = inv(U_bb) (z_b - U_bg x_g)
// Every sum has a fixed association (MFMA accumulators over the row chunks; blocks in index order inside a group of BB_GS,
// groups in index order): two runs of the same solve are bit-identical, whatever the launch mode.
//
// Dogleg(Cholesky()) is NOT offered: the reference factors with diagonal pivoting over the whole stacked matrix
// (dense_cholesky.jl:29-35) and reports RankDeficientException(rank) along that GLOBAL pivot order, which interleaves
// local and shared columns by the size of their pivots -- it does not split into "locals first".
#include <climits>

#include "lsq_solver.h"
#include "lsq_small64.h"
#include "lsq_cov.h"

constexpr int BB_R = 32;           // rows per streamed chunk
constexpr int BB_CS = BB_R + 2;    // column stride of the staged chunk (doubles)
constexpr int BB_MISC = 104;       // doubles behind M and W: y chunk (32) | right-hand side (64) | scalars (8)
constexpr int BB_GS = 64;          // blocks per first-level group of the contribution sum

// doubles of LDS per block (= per group of G wavefronts), na = nb + ng
static inline size_t bb_group_doubles(int na) { return 2 * (size_t)(16 * ((na + 15) / 16)) * S64_LS + BB_MISC; }
static inline size_t bb_contrib_len(int ng) { return (size_t)ng * (ng + 1) / 2 + ng; }

__global__ void k_bb_init(int *info) {
    if (threadIdx.x == 0) { info[0] = INT_MAX; info[1] = INT_MAX; info[2] = 0; info[3] = 0; }
}

// s64_chol16 stopped after the first kp < 16 columns of the diagonal block at o: rows < kp of the block become rows of U, rows
// >= kp keep the block's Schur complement (upper triangle), and W receives the row transformation T (lower triangular:
// [inv(U_11)' 0; -U_12' inv(U_11)' I]) with T G = [U_11 U_12; 0 S] -- applied to the tiles to the right it yields the rows of
// U and, below them, rows that are already updated.  Returns 0, or 1 + the index of the first pivot that is not positive.
__device__ __forceinline__ int bb_chol16_partial(double *__restrict__ M, double *__restrict__ W, int o, int kp, int lane) {
    const int c = lane & 15;
    const bool mat = lane < 16, idn = lane >= 16 && lane < 32;
    double u[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) u[r] = mat ? (r <= c ? M[(o + r) * S64_LS + o + c] : 0.0) : ((idn && r == c) ? 1.0 : 0.0);
    int bad = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if (j < kp) {                            // (wave-uniform)
            const double ajj = s64_readlane(u[j], j);
            bad = (bad == 0 && !(ajj > 0.0)) ? j + 1 : bad;
            const double rowj = u[j] * s64_rsqrt(ajj);
            u[j] = rowj;
#pragma unroll
            for (int i = j + 1; i < 16; ++i) u[i] = __builtin_fma(-s64_readlane(rowj, i), rowj, u[i]);
        }
    }
    if (mat) {
#pragma unroll
        for (int r = 0; r < 16; ++r) M[(o + r) * S64_LS + o + c] = r <= c ? u[r] : 0.0;
    } else if (idn) {
#pragma unroll
        for (int r = 0; r < 16; ++r) W[(o + r) * S64_LS + o + c] = c <= r ? u[r] : 0.0;
    }
    return bad;
}

// Unpivoted Cholesky of the first nloc columns of the (16 NT) x (16 NT) matrix in M (upper tiles), the blocked scheme of
// s64_chol / k_bd_solve on NT tile rows; the trailing (16 NT - nloc) square is left as the Schur complement of those columns.
// G wavefronts (wg = this one's index); every wavefront of the WORKGROUP must call it (barriers).  *fail: 0 on entry.
template <int G>
__device__ __forceinline__ void bb_chol_leading(double *__restrict__ M, double *__restrict__ W, int NT, int nloc, int *fail,
                                                int wg, int lane) {
    const int KB = (nloc + 15) >> 4;
    const int ij = lane & 15, kq = lane >> 4;
    for (int kb = 0; kb < KB; ++kb) {
        const int o = 16 * kb;
        const int kp = nloc - o < 16 ? nloc - o : 16;
        if (wg == 0) {
            const int bad = kp == 16 ? s64_chol16(M, W, o, lane) : bb_chol16_partial(M, W, o, kp, lane);
            if (bad && lane == 0 && *fail == 0) *fail = o + bad;
        }
        __syncthreads();
        const int nt = NT - 1 - kb;
        for (int q = wg; q < nt; q += G) {             // row panel: T G[o.., t] (kp = 16: U[o.., t] = inv(U_kk)' G[o.., t])
            const int t = kb + 1 + q;
            s64_v4d a = {0.0, 0.0, 0.0, 0.0};
            s64_tile_mma<false, false>(a, W, o, o, M, o, 16 * t, 1, lane);
            s64_tile_store<false>(M, o, 16 * t, a, 1.0, lane);
        }
        __syncthreads();
        for (int q = wg; q < nt * (nt + 1) / 2; q += G) {   // trailing tiles (ta <= tb) -= U[o .. o+kp, ta]' U[o .. o+kp, tb]
            int t = 0, r = q;
            while (r >= nt - t) { r -= nt - t; ++t; }
            const int ta = kb + 1 + t, tb = ta + r;
            s64_v4d a = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int k = kk * 4 + kq;
                const bool in = k < kp;                // (rows >= kp of the panel are not rows of U)
                const double av = in ? M[(o + k) * S64_LS + 16 * ta + ij] : 0.0;
                const double bv = in ? M[(o + k) * S64_LS + 16 * tb + ij] : 0.0;
                a = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, a, 0, 0, 0);
            }
            s64_tile_store<true>(M, 16 * ta, 16 * tb, a, -1.0, lane);
        }
        __syncthreads();
    }
}

template <int G>
__global__ void __launch_bounds__(256)
k_bb_eliminate(int B, int mb, int nb, int ng, const double *__restrict__ vals, const double *__restrict__ scale,
               const double *__restrict__ y, const double *__restrict__ damp, double *__restrict__ Uout,
               double *__restrict__ zout, double *__restrict__ contrib, int *__restrict__ info) {
    extern __shared__ double bb_lds[];
    constexpr int GT = 64 * G;                 // threads per block of the matrix
    constexpr int TPW = G == 4 ? 3 : 1;        // upper tiles per wavefront (10 tiles over 4 wavefronts / 1 tile)
    constexpr int CP = GT / 32;                // columns per load pass
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wg = G == 4 ? __builtin_amdgcn_readfirstlane(wv) : 0;      // wavefront inside its group
    const int gt = G == 4 ? tid : lane;                                  // thread inside its group
    const int b = G == 4 ? (int)blockIdx.x : (int)blockIdx.x * 4 + wv;
    const bool live = b < B;
    const int na = nb + ng;
    const int NT = (na + 15) >> 4, ncp = 16 * NT;
    const int msz = ncp * S64_LS;
    double *M = bb_lds + (G == 4 ? 0 : wv) * (size_t)(2 * msz + BB_MISC);
    double *W = M + msz;                       // chunk staging while streaming, then the row transformations of the factorisation
    double *ch = W;
    double *ych = W + msz;
    double *rv = ych + 32;
    int *misc_i = (int *)(rv + 64 + 1);        // [1] first failing local column
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
    const bool rtile = wg < NT;                // this wavefront forms rows 16 wg .. of r = A'y

    // ---- stream A_b = [J_b C_b]: G (upper tiles) and r ----
    // column c < nb: the block's own column (mb contiguous doubles); nb <= c < na: rows b*mb .. of border column c - nb
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
            double v = 0.0;
            if (ok && c < nb) v = vals[vbase + (size_t)c * mb + row];
            else if (ok && c < na) v = vals[cbase + (size_t)(c - nb) * m + row];
            reg[p] = v;
        }
        if (gt < 32) yreg = ok ? y[ybase + row] : 0.0;
    };
    s64_v4d acc[TPW], racc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < TPW; ++q) acc[q] = s64_v4d{0.0, 0.0, 0.0, 0.0};
    const int nch = (mb + BB_R - 1) / BB_R;
    load(0);
    for (int c = 0; c < nch; ++c) {
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int col = c0 + p * CP;
            if (col < ncp) ch[col * BB_CS + lr] = reg[p];      // (columns na .. ncp-1: zeros)
        }
        if (gt < 32) ych[gt] = yreg;
        __syncthreads();
        if (c + 1 < nch) load((c + 1) * BB_R);                 // in flight during the tile products
#pragma unroll
        for (int ks = 0; ks < BB_R / 4; ++ks) {
            const int kk = 4 * ks + kq;
#pragma unroll
            for (int q = 0; q < TPW; ++q) {
                if (has[q]) {
                    const double a = ch[(16 * ti[q] + ij) * BB_CS + kk];
                    const double bb = ch[(16 * tj[q] + ij) * BB_CS + kk];
                    acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bb, acc[q], 0, 0, 0);
                }
            }
            if (rtile) {
                const double a = ch[(16 * wg + ij) * BB_CS + kk];
                const double bb = ij == 0 ? ych[kk] : 0.0;
                racc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bb, racc, 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // ---- G (column-scaled handle: S G_V S, r = S r_V; S includes the ng border factors) into M, r into rv ----
    auto sc = [&](int k) {
        if (!scale || !live || k >= na) return 1.0;
        return k < nb ? scale[(size_t)b * nb + k] : scale[(size_t)B * nb + (k - nb)];
    };
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
    if (gt == 0) misc_i[1] = 0;
    __syncthreads();
    if (gt < ncp) {
        if (!live || gt >= na) M[gt * S64_LS + gt] = 1.0;                          // padding: identity
        else if (gt < nb) M[gt * S64_LS + gt] += damp[(size_t)b * nb + gt];       // (the border's damping: k_bb_schur)
    }
    __syncthreads();

    // ---- dense_cholesky.jl:43-59 on the first nb columns: G + D = U'U, unpivoted; the corner keeps the Schur complement ----
    bb_chol_leading<G>(M, W, NT, nb, &misc_i[1], wg, lane);
    const int fail = misc_i[1];
    if (!live) return;                         // (no barrier below)
    if (fail && gt == 0) {
        atomicMin(&info[0], b * nb + fail);
        atomicMin(&info[1], b);
    }
    const size_t L = (size_t)ng * (ng + 1) / 2 + ng;
    double *cb = contrib + (size_t)b * L;
    if (wg == 0) {
        // U_bb'z = r_b, and r_g - U_bg'z in the lanes behind: one wavefront, lane = unknown, the pivot row broadcast with v_readlane
        const bool in = lane < na;
        const int li = in ? lane : 0;
        const double dinv = lane < nb ? 1.0 / M[li * S64_LS + li] : 1.0;
        double z = in ? rv[li] : 0.0;
        for (int k = 0; k < nb; ++k) {
            const double u = M[k * S64_LS + li];
            const double zk = s64_readlane(z * dinv, k);
            if (lane == k) z = zk;
            else if (in && lane > k) z -= u * zk;
        }
        if (lane < nb) zout[(size_t)b * nb + lane] = z;
        else if (in) cb[L - ng + (lane - nb)] = z;
    }
    double *ub = Uout + (size_t)b * nb * na;
    for (int e = gt; e < nb * na; e += GT) {   // rows of U: [U_bb U_bg], zeros below the diagonal
        const int k = e / na, c = e - k * na;
        ub[e] = c >= k ? M[k * S64_LS + c] : 0.0;
    }
    for (int e = gt; e < ng * ng; e += GT) {   // the corner, upper triangle by rows
        const int i = e / ng, j = e - i * ng;
        if (j >= i) cb[(size_t)i * ng - (size_t)i * (i - 1) / 2 + (j - i)] = M[(nb + i) * S64_LS + nb + j];
    }
}

// partial[p][e] = sum of contrib[b][e] over the blocks b of group p (BB_GS consecutive blocks), in index order
__global__ void __launch_bounds__(256)
k_bb_reduce(int B, int L, const double *__restrict__ contrib, double *__restrict__ partial) {
    const int e = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y;
    if (e >= L) return;
    const int b0 = p * BB_GS, b1 = b0 + BB_GS < B ? b0 + BB_GS : B;
    double s = 0.0;
    for (int b = b0; b < b1; ++b) s += contrib[(size_t)b * L + e];
    partial[(size_t)p * L + e] = s;
}

// S = sum of the `count` contributions (index order) + D_g, S = U'U, U'z = r, U x_g = z
__global__ void __launch_bounds__(256)
k_bb_schur(int count, int ng, int col0, int nblocks, const double *__restrict__ contrib, const double *__restrict__ damp_g,
           double *__restrict__ xg, int *__restrict__ info) {
    extern __shared__ double bb_lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wg = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int NT = (ng + 15) >> 4, ncp = 16 * NT;
    const int msz = ncp * S64_LS;
    double *M = bb_lds;
    double *W = M + msz;
    double *rv = W + msz;                      // 64
    int *misc_i = (int *)(rv + 64);
    const int T = ng * (ng + 1) / 2, L = T + ng;
    for (int e = tid; e < ncp * ncp; e += 256) {   // padding: identity; everything the tile products may read is defined
        const int i = e / ncp, j = e - i * ncp;
        M[i * S64_LS + j] = (i == j && i >= ng) ? 1.0 : 0.0;
    }
    if (tid == 0) misc_i[0] = 0;
    __syncthreads();
    for (int e = tid; e < L; e += 256) {
        double s = 0.0;
        for (int q = 0; q < count; ++q) s += contrib[(size_t)q * L + e];
        if (e >= T) rv[e - T] = s;
        else {
            int i = 0, r = e;
            while (r >= ng - i) { r -= ng - i; ++i; }
            if (r == 0) s += damp_g[i];
            M[i * S64_LS + i + r] = s;
        }
    }
    __syncthreads();
    bb_chol_leading<4>(M, W, NT, ncp, &misc_i[0], wg, lane);
    const int fail = misc_i[0];
    if (wg != 0) return;
    if (fail) {
        if (lane == 0) {                       // (a smaller column recorded by k_bb_eliminate stays)
            atomicMin(&info[0], col0 + fail);
            atomicMin(&info[1], nblocks);
        }
        return;
    }
    const bool in = lane < ncp;
    const int li = in ? lane : 0;
    const double dinv = 1.0 / M[li * S64_LS + li];
    double z = lane < ng ? rv[li] : 0.0;
#pragma unroll 4
    for (int k = 0; k < ncp; ++k) {
        const double u = M[k * S64_LS + li];
        const double zk = s64_readlane(z * dinv, k);
        if (lane == k) z = zk;
        else if (in && lane > k) z -= u * zk;
    }
#pragma unroll 4
    for (int k = ncp - 1; k >= 0; --k) {
        const double u = M[li * S64_LS + k];
        const double xk = s64_readlane(z * dinv, k);
        if (lane == k) z = xk;
        else if (lane < k) z -= u * xk;
    }
    if (lane < ng) xg[lane] = z;
}

// x_b = inv(U_bb) (z_b - U_bg x_g): one wavefront per block, U_b staged in LDS with an odd row stride
__global__ void __launch_bounds__(64)
k_bb_back(int nb, int ng, const double *__restrict__ Uin, const double *__restrict__ zin, const double *__restrict__ xg,
          double *__restrict__ x) {
    extern __shared__ double bb_lds[];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int na = nb + ng, ld = na | 1;
    double *sU = bb_lds;
    double *sx = sU + nb * ld;
    const double *ub = Uin + (size_t)b * nb * na;
    for (int e = lane; e < nb * na; e += 64) {
        const int k = e / na, c = e - k * na;
        sU[k * ld + c] = ub[e];
    }
    if (lane < ng) sx[lane] = xg[lane];
    __syncthreads();
    const bool in = lane < nb;
    const int li = in ? lane : 0;
    double t = in ? zin[(size_t)b * nb + li] : 0.0;
    for (int c = 0; c < ng; ++c) t -= sU[li * ld + nb + c] * sx[c];
    const double dinv = 1.0 / sU[li * ld + li];
    for (int k = nb - 1; k >= 0; --k) {
        const double u = sU[li * ld + k];
        const double xk = s64_readlane(t * dinv, k);
        if (lane == k) t = xk;
        else if (lane < k) t -= u * xk;
    }
    if (in) x[(size_t)b * nb + lane] = t;
}

// ---- covariance (lsq_solver_covariance on a bordered handle): s^2 inv(J'J), the B diagonal blocks of the locals and the
// ng x ng block of the shared parameters.  With the elimination above run WITHOUT damping, S = U_g'U_g is the Schur complement
// of the locals in J'J and
//     Cov_gg = s^2 inv(S),      Cov_bb = s^2 X_b X_b' + W_b Cov_gg W_b',   X_b = inv(U_bb),  W_b = X_b U_bg = inv(G_bb) G_bg
// (the cross blocks -W_b Cov_gg are not formed).  k_bb_eliminate and k_bb_reduce run unchanged; two new kernels follow them in
// stream order, nothing is exchanged inside a launch, every sum has a fixed association, no floating-point atomics.

// S = sum of the `count` contributions (index order), S = U'U, Cov_gg = s2 inv(U) inv(U)' -> cg (always) and covg / seg (null
// or the caller's).  One workgroup.
__global__ void __launch_bounds__(256)
k_bb_cov_schur(int count, int ng, int col0, int nblocks, const double *__restrict__ contrib, double s2, double *__restrict__ cg,
               double *__restrict__ covg, double *__restrict__ seg, int *__restrict__ info) {
    extern __shared__ double bb_lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wg = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int NT = (ng + 15) >> 4, ncp = 16 * NT;
    const int msz = ncp * S64_LS;
    double *M = bb_lds;
    double *W = M + msz;
    int *misc_i = (int *)(W + msz);
    const int T = ng * (ng + 1) / 2;
    for (int e = tid; e < ncp * ncp; e += 256) {   // padding: identity; everything the tile products may read is defined
        const int i = e / ncp, j = e - i * ncp;
        M[i * S64_LS + j] = (i == j && i >= ng) ? 1.0 : 0.0;
        W[i * S64_LS + j] = 0.0;
    }
    if (tid == 0) misc_i[0] = 0;
    __syncthreads();
    const int L = T + ng;
    for (int e = tid; e < T; e += 256) {
        double s = 0.0;
        for (int q = 0; q < count; ++q) s += contrib[(size_t)q * L + e];
        int i = 0, r = e;
        while (r >= ng - i) { r -= ng - i; ++i; }
        M[i * S64_LS + i + r] = s;
    }
    __syncthreads();
    bb_chol_leading<4>(M, W, NT, ncp, &misc_i[0], wg, lane);
    const int fail = misc_i[0];
    if (fail) {                                // (the same answer in every thread; a smaller column recorded by k_bb_eliminate stays)
        if (tid == 0) {
            atomicMin(&info[0], col0 + fail);
            atomicMin(&info[1], nblocks);
        }
        return;
    }
    cov_inv_levels<4>(M, W, NT, wg, lane);
    for (int t = wg; t < NT * (NT + 1) / 2; t += 4) {
        int ti = 0, r = t;
        while (r >= NT - ti) { r -= NT - ti; ++ti; }
        const int tj = ti + r;
        const s64_v4d a = cov_tile(W, W, NT, ti, tj, lane);
        cov_store(cg, nullptr, ng, ti, tj, a, s2, lane);
        cov_store(covg, seg, ng, ti, tj, a, s2, lane);
    }
}

// Cov_bb per block, the geometry of k_bb_eliminate (na = nb + ng > 16: one workgroup per block, else one wavefront per block,
// four per workgroup).  The rows [U_bb U_bg] of the block are completed to the na x na upper triangular Uh = [U_bb U_bg; 0 I],
// whose inverse is [X_b -W_b; 0 I]: Y = inv(Uh)' by lsq_cov.h, and with K = diag(s2 I_nb, Cov_gg)
//     Cov_bb = the leading nb x nb block of Y' K Y.
// P = K Y differs from s2 Y only in the ng rows of the shared parameters (an ng x nb product, one thread per entry, Cov_gg read
// from global memory); then the upper tiles of Y'P on the MFMA unit, stored with their mirrors.
template <int G>
__global__ void __launch_bounds__(256)
k_bb_cov_back(int B, int nb, int ng, const double *__restrict__ Uin, const double *__restrict__ cg, double s2,
              double *__restrict__ cov, double *__restrict__ se) {
    extern __shared__ double bb_lds[];
    constexpr int GT = 64 * G;
    constexpr int TPW = G == 4 ? 3 : 1;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wg = G == 4 ? __builtin_amdgcn_readfirstlane(wv) : 0;
    const int gt = G == 4 ? tid : lane;
    const int b = G == 4 ? (int)blockIdx.x : (int)blockIdx.x * 4 + wv;
    const bool live = b < B;
    const int na = nb + ng;
    const int NT = (na + 15) >> 4, ncp = 16 * NT;
    const int NTB = (nb + 15) >> 4, nbp = 16 * NTB;    // the tile rows / columns that hold locals
    const int msz = ncp * S64_LS;
    double *M = bb_lds + (G == 4 ? 0 : wv) * (size_t)(2 * msz);
    double *W = M + msz;
    const double *ub = Uin + (live ? (size_t)b * nb * na : 0);
    for (int e = gt; e < ncp * ncp; e += GT) {         // Uh (padding, and a workgroup's unused wavefronts: identity)
        const int k = e / ncp, c = e - k * ncp;
        double v = k == c ? 1.0 : 0.0;
        if (live && k < nb && c < na) v = ub[k * na + c];
        M[k * S64_LS + c] = v;
        W[k * S64_LS + c] = 0.0;
    }
    __syncthreads();
    cov_diaginv_t<G>(M, W, NT, wg, lane);
    __syncthreads();
    cov_inv_levels<G>(M, W, NT, wg, lane);
    for (int e = gt; e < ncp * nbp; e += GT) {         // P = K Y, the columns of the locals
        const int k = e / nbp, j = e - k * nbp;
        double v = 0.0;
        if (k < nb) v = s2 * W[k * S64_LS + j];
        else if (k < na)
            for (int l = 0; l < ng; ++l) v += cg[(k - nb) * ng + l] * W[(nb + l) * S64_LS + j];
        M[k * S64_LS + j] = v;
    }
    __syncthreads();
    if (!live) return;                                 // (no barrier below)
    double *cb = cov ? cov + (size_t)b * nb * nb : nullptr;
    double *sb = se ? se + (size_t)b * nb : nullptr;
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
        const int t = wg + G * q;
        if (t < NTB * (NTB + 1) / 2) {
            int ti = 0, r = t;
            while (r >= NTB - ti) { r -= NTB - ti; ++ti; }
            const int tj = ti + r;
            const s64_v4d a = cov_tile(W, M, NT, ti, tj, lane);
            cov_store(cb, sb, nb, ti, tj, a, 1.0, lane);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
extern "C" int lsq_blockdiag_bordered_create(lsq_ctx *c, int nblocks, int mb, int nb, int ng, lsq_mat **out) {
    LSQ_RANGE("lsq_blockdiag_bordered_create");
    if (!c || !out) { lsq_set_error("lsq_blockdiag_bordered_create: null argument"); return LSQ_EARG; }
    if (nblocks < 1 || mb < 1 || nb < 1 || ng < 1) {
        lsq_set_error("lsq_blockdiag_bordered_create: needs nblocks >= 1, mb >= 1, nb >= 1, ng >= 1 (got %d, %d, %d, %d)",
                      nblocks, mb, nb, ng);
        return LSQ_EDIM;
    }
    const long long m = (long long)nblocks * mb, nloc = (long long)nblocks * nb, n = nloc + ng;
    if (m > INT_MAX || n > INT_MAX || (double)m * ((double)nb + ng) > 2147483000.0) {
        lsq_set_error("lsq_blockdiag_bordered_create: %d blocks of %d x %d with %d shared columns do not fit 32-bit indices",
                      nblocks, mb, nb, ng);
        return LSQ_EDIM;
    }
    const long long nnz = m * (nb + ng);
    try {
        std::vector<int> colptr((size_t)n + 1), rowval((size_t)nnz);
        for (long long j = 0; j <= nloc; ++j) colptr[(size_t)j] = (int)(j * mb);
        for (long long j = 1; j <= ng; ++j) colptr[(size_t)(nloc + j)] = (int)(nloc * mb + j * m);
        for (int b = 0; b < nblocks; ++b)
            for (int j = 0; j < nb; ++j) {
                int *rv = rowval.data() + ((size_t)b * nb + j) * mb;
                for (int i = 0; i < mb; ++i) rv[i] = b * mb + i;
            }
        for (int j = 0; j < ng; ++j) {
            int *rv = rowval.data() + (size_t)(nloc * mb) + (size_t)j * m;
            for (long long i = 0; i < m; ++i) rv[i] = (int)i;
        }
        LSQ_TRY(lsq_csc_create(c, (int)m, (int)n, colptr.data(), rowval.data(), out));
    } catch (const std::bad_alloc &) {
        lsq_set_error("lsq_blockdiag_bordered_create: out of host memory while building the pattern");
        return LSQ_EHIP;
    }
    (*out)->br_blocks = nblocks;
    (*out)->br_mb = mb;
    (*out)->br_nb = nb;
    (*out)->br_ng = ng;
    return LSQ_OK;
}

extern "C" int lsq_mat_bordered_info(const lsq_mat *J, int *nblocks, int *mb, int *nb, int *ng) {
    if (!J) { lsq_set_error("lsq_mat_bordered_info: null argument"); return LSQ_EARG; }
    if (nblocks) *nblocks = J->br_blocks;
    if (mb) *mb = J->br_mb;
    if (nb) *nb = J->br_nb;
    if (ng) *ng = J->br_ng;
    return LSQ_OK;
}

int lsq_bordered_refuse_dogleg() {
    lsq_set_error("Dogleg(Cholesky()) is not available on a bordered block-diagonal Jacobian: the reference's pivoted "
                  "factorisation orders local and shared columns together, which does not split into blocks. "
                  "Use LevenbergMarquardt(Cholesky()) or LSMR()");
    return LSQ_EARG;
}

int lsq_bordered_solver_alloc(lsq_solver *s, const lsq_mat *J) {
    if (J->br_nb + J->br_ng > 64) {
        lsq_set_error("Cholesky() on a bordered block-diagonal Jacobian needs nb + ng <= 64 (got nb = %d, ng = %d): one block's "
                      "augmented normal matrix must fit the 64 x 64 in-LDS factorisation. Use LSMR()", J->br_nb, J->br_ng);
        return LSQ_EARG;
    }
    if (!s->for_lm) return lsq_bordered_refuse_dogleg();
    s->br_blocks = J->br_blocks;
    s->br_mb = J->br_mb;
    s->br_nb = J->br_nb;
    s->br_ng = J->br_ng;
    const size_t B = (size_t)J->br_blocks, nb = (size_t)J->br_nb, na = nb + J->br_ng, L = bb_contrib_len(J->br_ng);
    const size_t groups = B > (size_t)BB_GS ? (B + BB_GS - 1) / BB_GS : 0;
    // U (B nb na) | z (B nb) | contributions (B L) | first-level partial sums (groups L)
    s->work_elems = B * (nb * (na + 1) + L) + groups * L;
    LSQ_HIP(hipMalloc(&s->d_work, s->work_elems * sizeof(double)));
    LSQ_HIP(hipMalloc(&s->d_info, 4 * sizeof(int)));
    return LSQ_OK;
}

template <int G>
static int bb_eliminate(lsq_ctx *c, lsq_solver *s, lsq_mat *J, const double *d_y, const double *d_damp, double *U, double *z,
                        double *contrib) {
    const int B = s->br_blocks, na = s->br_nb + s->br_ng;
    const size_t lds = (G == 4 ? 1 : 4) * bb_group_doubles(na) * sizeof(double);
    LSQ_TRY(lsq_set_lds(c, (const void *)k_bb_eliminate<G>, lds));
    const int grid = G == 4 ? B : (B + 3) / 4;
    LSQ_LAUNCH((k_bb_eliminate<G>), dim3(grid), dim3(256), lds, c->stream, B, s->br_mb, s->br_nb, s->br_ng,
               (const double *)J->csc.d_val, J->d_colscale, d_y, d_damp, U, z, contrib, s->d_info);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

// dense_cholesky.jl:43-59 (damped, unpivoted, LM) on the stacked system
int lsq_bordered_solve(lsq_solver *s, lsq_mat *J, const double *d_y, const double *d_damp, double *d_x, int *nmul) {
    lsq_ctx *c = s->ctx;
    if (!d_damp) return lsq_bordered_refuse_dogleg();
    if (J->kind != LSQ_MAT_CSC || J->br_blocks != s->br_blocks || J->br_mb != s->br_mb || J->br_nb != s->br_nb ||
        J->br_ng != s->br_ng || J->m != s->m || J->n != s->n) {
        lsq_set_error("cholesky: this solver was allocated for a bordered block-diagonal Jacobian of %d blocks of %d x %d "
                      "with %d shared columns", s->br_blocks, s->br_mb, s->br_nb, s->br_ng);
        return LSQ_EDIM;
    }
    LSQ_TRY(lsq_ensure_csc(J));        // (a device-side g! may have written the product mirrors only)
    const int B = s->br_blocks, nb = s->br_nb, ng = s->br_ng, na = nb + ng;
    const size_t L = bb_contrib_len(ng);
    double *U = s->d_work, *z = U + (size_t)B * nb * na, *contrib = z + (size_t)B * nb, *partial = contrib + (size_t)B * L;
    LSQ_LAUNCH(k_bb_init, dim3(1), dim3(64), 0, c->stream, s->d_info);
    if (na > 16) LSQ_TRY(bb_eliminate<4>(c, s, J, d_y, d_damp, U, z, contrib));
    else LSQ_TRY(bb_eliminate<1>(c, s, J, d_y, d_damp, U, z, contrib));
    int count = B;
    const double *src = contrib;
    if (B > BB_GS) {
        count = (B + BB_GS - 1) / BB_GS;
        LSQ_LAUNCH(k_bb_reduce, dim3((unsigned)((L + 255) / 256), (unsigned)count), dim3(256), 0, c->stream, B, (int)L,
                   (const double *)contrib, partial);
        src = partial;
    }
    const size_t lds2 = (2 * (size_t)(16 * ((ng + 15) / 16)) * S64_LS + 64 + 8) * sizeof(double);
    LSQ_TRY(lsq_set_lds(c, (const void *)k_bb_schur, lds2));
    LSQ_LAUNCH(k_bb_schur, dim3(1), dim3(256), lds2, c->stream, count, ng, B * nb, B, src, d_damp + (size_t)B * nb,
               d_x + (size_t)B * nb, s->d_info);
    const size_t lds3 = ((size_t)nb * (na | 1) + 64) * sizeof(double);
    LSQ_LAUNCH(k_bb_back, dim3(B), dim3(64), lds3, c->stream, nb, ng, (const double *)U, (const double *)z,
               (const double *)(d_x + (size_t)B * nb), d_x);
    LSQ_HIP(hipGetLastError());
    s->last_bd_path = 4;
    s->last_bd_block = -1;
    int st4[4] = {0, 0, 0, 0};
    LSQ_TRY(lsq_read_ints(c, s->d_info, s->d_info + 1, nullptr, nullptr, st4));
    if (nmul) *nmul = 1;
    if (st4[1] != INT_MAX) {
        s->last_bd_block = st4[1];
        lsq_set_error("PosDefException: matrix is not positive definite; Cholesky failed at %d", st4[0]);
        return LSQ_ENOTPD;
    }
    return LSQ_OK;
}

template <int G>
static int bb_cov_back(lsq_ctx *c, lsq_solver *s, const double *U, const double *cg, double s2, double *d_cov, double *d_stderr) {
    const int B = s->br_blocks, na = s->br_nb + s->br_ng;
    const size_t lds = (G == 4 ? 1 : 4) * 2 * (size_t)(16 * ((na + 15) / 16)) * S64_LS * sizeof(double);
    LSQ_TRY(lsq_set_lds(c, (const void *)k_bb_cov_back<G>, lds));
    const int grid = G == 4 ? B : (B + 3) / 4;
    LSQ_LAUNCH((k_bb_cov_back<G>), dim3(grid), dim3(256), lds, c->stream, B, s->br_nb, s->br_ng, U, cg, s2, d_cov, d_stderr);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

// lsq_solver_covariance on a bordered handle: d_cov = B nb x nb blocks, then ng x ng; d_stderr = n
int lsq_bordered_covariance(lsq_solver *s, lsq_mat *J, const double *d_f, double *d_cov, double *d_stderr, int *h_info) {
    lsq_ctx *c = s->ctx;
    if (J->kind != LSQ_MAT_CSC || J->br_blocks != s->br_blocks || J->br_mb != s->br_mb || J->br_nb != s->br_nb ||
        J->br_ng != s->br_ng || J->m != s->m || J->n != s->n) {
        lsq_set_error("lsq_solver_covariance: this solver was allocated for a bordered block-diagonal Jacobian of %d blocks of "
                      "%d x %d with %d shared columns", s->br_blocks, s->br_mb, s->br_nb, s->br_ng);
        return LSQ_EARG;
    }
    if (d_f && s->m <= s->n) {
        lsq_set_error("lsq_solver_covariance: the residual variance sum(f.^2) / (m - n) needs m > n (got m = %d, n = %d); "
                      "pass d_f = NULL for the unscaled inv(J'J)", s->m, s->n);
        return LSQ_EARG;
    }
    LSQ_HIP(hipSetDevice(c->device));
    LSQ_TRY(lsq_ensure_csc(J));        // (a device-side g! may have written the product mirrors only)
    const int B = s->br_blocks, nb = s->br_nb, ng = s->br_ng, na = nb + ng;
    const size_t nz = (size_t)s->m > (size_t)B * nb ? (size_t)s->m : (size_t)B * nb;      // zeros: damping (B nb) and right-hand side (m)
    if (!s->d_cov_buf) {
        LSQ_HIP(hipMalloc(&s->d_cov_buf, (nz + (size_t)ng * ng) * sizeof(double)));
        LSQ_HIP(hipMemsetAsync(s->d_cov_buf, 0, nz * sizeof(double), c->stream));
    }
    const double *zero = s->d_cov_buf;
    double *cg = s->d_cov_buf + nz;
    double s2 = 1.0;
    if (d_f) {                         // the library's deterministic reduction (block partials in a fixed order)
        double ssq = 0.0;
        LSQ_TRY(lsq_sumsq(c, s->m, d_f, &ssq));
        s2 = ssq / (double)(s->m - s->n);
    }
    const size_t L = bb_contrib_len(ng);
    double *U = s->d_work, *z = U + (size_t)B * nb * na, *contrib = z + (size_t)B * nb, *partial = contrib + (size_t)B * L;
    LSQ_LAUNCH(k_bb_init, dim3(1), dim3(64), 0, c->stream, s->d_info);
    if (na > 16) LSQ_TRY(bb_eliminate<4>(c, s, J, zero, zero, U, z, contrib));
    else LSQ_TRY(bb_eliminate<1>(c, s, J, zero, zero, U, z, contrib));
    int count = B;
    const double *src = contrib;
    if (B > BB_GS) {
        count = (B + BB_GS - 1) / BB_GS;
        LSQ_LAUNCH(k_bb_reduce, dim3((unsigned)((L + 255) / 256), (unsigned)count), dim3(256), 0, c->stream, B, (int)L,
                   (const double *)contrib, partial);
        src = partial;
    }
    const size_t lds2 = (2 * (size_t)(16 * ((ng + 15) / 16)) * S64_LS + 8) * sizeof(double);
    LSQ_TRY(lsq_set_lds(c, (const void *)k_bb_cov_schur, lds2));
    LSQ_LAUNCH(k_bb_cov_schur, dim3(1), dim3(256), lds2, c->stream, count, ng, B * nb, B, src, s2, cg,
               d_cov ? d_cov + (size_t)B * nb * nb : nullptr, d_stderr ? d_stderr + (size_t)B * nb : nullptr, s->d_info);
    if (na > 16) LSQ_TRY(bb_cov_back<4>(c, s, U, cg, s2, d_cov, d_stderr));
    else LSQ_TRY(bb_cov_back<1>(c, s, U, cg, s2, d_cov, d_stderr));
    s->last_bd_path = 4;
    s->last_bd_block = -1;
    int st4[4] = {0, 0, 0, 0};
    LSQ_TRY(lsq_read_ints(c, s->d_info, s->d_info + 1, nullptr, nullptr, st4));
    if (h_info) h_info[0] = 0;
    if (st4[1] != INT_MAX) {
        s->last_bd_block = st4[1];
        if (h_info) h_info[0] = st4[0];
        lsq_set_error("PosDefException: matrix is not positive definite; Cholesky failed at %d", st4[0]);
        return LSQ_ENOTPD;
    }
    return LSQ_OK;
}
