// Block-diagonal Jacobians J = blkdiag(J_1 .. J_B), every block dense mb x nb with nb <= 64: the handle
// (lsq_blockdiag_create: a CSC handle that also knows its block shape) and the Cholesky() solver on it.
//
// J'J + D is block-diagonal, so the normal equations of dense_cholesky.jl:29-59 are B independent nb x nb problems and one
// solve is ONE pass over the values.  Per block b: G_b = J_b'J_b (+ diag(damp_b)), r_b = J_b'y_b, factor, two
// triangular solves, write x_b -- everything after the Gram matrix stays in LDS / registers and a block never talks to
// another block (no exchange between workgroups, no waits).  The only words shared between blocks are integers:
//   info[0]  LM:     min over the failing blocks of b * nb + k_b, the 1-based column at which dpotrf of the STACKED matrix
//                    stops (the dense factorisation reaches the lowest-numbered failing block first)
//   info[1]  the lowest-numbered block that failed (LM: not positive definite; Dogleg: rank deficient)
//   info[2]  Dogleg: sum over the blocks of nb - rank_b.  Diagonal pivoting on the stacked matrix restricted to one block is
//            that block's own greedy pivoting and blocks never update each other; with the reference's tol = 0
//            (cholesky!(.., Val(true)) passes tol = 0.0: the stop rule is "largest remaining pivot <= 0") the stacked dpstrf
//            stops early iff some block's own pivoted factorisation does, and its rank is the sum of the block ranks.
// Sums are formed in a fixed order (MFMA accumulators over the row chunks, no floating-point atomics): two runs of the same
// solve are bit-identical.
//
// Geometry: 16 < nb <= 64: one 256-thread workgroup per block (G = 4 wavefronts);  nb <= 16: one wavefront per block, four
// blocks per workgroup (G = 1).  J_b is streamed in chunks of 32 rows, loaded down the columns (a block's column is mb
// contiguous doubles), staged in LDS as [column][row] with a column stride of 34 doubles (the 16 x 4 operand reads of
// v_mfma_f64_16x16x4_f64 then hit 32 different banks per half wavefront); the next chunk's loads are in flight while the
// upper-triangle 16 x 16 tiles of G_b are accumulated.  y_b rides along as one more operand column (its own tile column,
// so that nb = 16, 32, 48, 64 need no 17th column).
#include <climits>

#include "lsq_solver.h"
#include "lsq_small64.h"

constexpr int BD_R = 32;           // rows per streamed chunk
constexpr int BD_CS = BD_R + 2;    // column stride of the staged chunk (doubles)
constexpr int BD_MISC = 104;       // doubles behind M and W: y chunk (32) | right-hand side (64) | scalars (8)
constexpr double BD_MIN_DIAGONAL = 1e-6, BD_MAX_DIAGONAL = 1e32;   // levenberg_marquardt.jl:85 (per-block damping, `delta`)

// doubles of LDS per block (= per group of G wavefronts)
static inline size_t bd_group_doubles(int nb) { return 2 * (size_t)(16 * ((nb + 15) / 16)) * S64_LS + BD_MISC; }

__global__ void k_bd_init(int *info) {
    if (threadIdx.x == 0) { info[0] = INT_MAX; info[1] = INT_MAX; info[2] = 0; info[3] = 0; }
}

template <int G, bool PIVOT>
__global__ void __launch_bounds__(256)
k_bd_solve(int B, int mb, int nb, const double *__restrict__ vals, const double *__restrict__ scale,
           const double *__restrict__ y, const double *__restrict__ damp, double *__restrict__ x, int *__restrict__ info,
           const int *__restrict__ active, int *__restrict__ binfo, double *__restrict__ r_out,
           double *__restrict__ diag_out, const double *__restrict__ delta) {
    // The last five are the batched trust-region loop's (lsq_batched.hip); all null = lsq_blockdiag_solve, unchanged:
    //   active    per-block mask: a workgroup none of whose blocks is active returns before loading anything; an inactive
    //             block that shares its workgroup with active ones (G = 1) runs as padding (no loads, no stores)
    //   binfo     per-block verdict INSTEAD of the cross-block words of `info`: 0, or LM: the 1-based column at which the block's
    //             dpotrf stops / Dogleg: nb - rank_b
    //   r_out     r_b = J_b'y_b (the gradient of levenberg_marquardt.jl:102 / dogleg.jl:99 when y = fcur)
    //   diag_out  diag(J_b'J_b) = colsumabs2(J_b) (levenberg_marquardt.jl:82 / dogleg.jl:85) before any damping
    //   delta     LM with one trust region per block (damp == nullptr): the damping of levenberg_marquardt.jl:84-86 is formed
    //             here from the block's own diagonal -- clamp(dtd_b, MIN * mean(dtd_b), MAX * mean(dtd_b)) * (1 / delta_b)
    extern __shared__ double bd_lds[];
    constexpr int GT = 64 * G;                 // threads per block of the matrix
    constexpr int TPW = G == 4 ? 3 : 1;        // upper tiles per wavefront (10 tiles over 4 wavefronts / 1 tile)
    constexpr int CP = GT / 32;                // columns per load pass
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wg = G == 4 ? __builtin_amdgcn_readfirstlane(wv) : 0;      // wavefront inside its group
    const int gt = G == 4 ? tid : lane;                                  // thread inside its group
    const int b = G == 4 ? (int)blockIdx.x : (int)blockIdx.x * 4 + wv;
    if (active) {
        bool any = false;
        for (int q = 0; q < (G == 4 ? 1 : 4); ++q) {
            const int bq = G == 4 ? (int)blockIdx.x : (int)blockIdx.x * 4 + q;
            any = any || (bq < B && active[bq] != 0);
        }
        if (!any) return;              // (the same answer in every thread of the workgroup)
    }
    const bool live = b < B && (!active || active[b] != 0);
    const int NT = (nb + 15) >> 4, ncp = 16 * NT;
    const int msz = ncp * S64_LS;
    double *M = bd_lds + (G == 4 ? 0 : wv) * (size_t)(2 * msz + BD_MISC);
    double *W = M + msz;                       // chunk staging while streaming, then inv(U_kk)' (LM) / the factor (Dogleg)
    double *ch = W;
    double *ych = W + msz;
    double *rv = ych + 32;
    double *misc_d = rv + 64;                  // [0] pivot value
    int *misc_i = (int *)(misc_d + 1);         // [0] pivot index, [1] first failing column (LM)
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
    const bool rtile = wg < NT;                // this wavefront forms rows 16 wg .. of r = J'y

    // ---- stream J_b: G (upper tiles) and r ----
    const size_t vbase = live ? (size_t)b * mb * nb : 0;
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
    s64_v4d acc[TPW], racc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < TPW; ++q) acc[q] = s64_v4d{0.0, 0.0, 0.0, 0.0};
    const int nch = (mb + BD_R - 1) / BD_R;
    load(0);
    for (int c = 0; c < nch; ++c) {
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int col = c0 + p * CP;
            if (col < ncp) ch[col * BD_CS + lr] = reg[p];      // (columns nb .. ncp-1: zeros)
        }
        if (gt < 32) ych[gt] = yreg;
        __syncthreads();
        if (c + 1 < nch) load((c + 1) * BD_R);                 // in flight during the tile products
#pragma unroll
        for (int ks = 0; ks < BD_R / 4; ++ks) {
            const int kk = 4 * ks + kq;
#pragma unroll
            for (int q = 0; q < TPW; ++q) {
                if (has[q]) {
                    const double a = ch[(16 * ti[q] + ij) * BD_CS + kk];
                    const double bb = ch[(16 * tj[q] + ij) * BD_CS + kk];
                    acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bb, acc[q], 0, 0, 0);
                }
            }
            if (rtile) {
                const double a = ch[(16 * wg + ij) * BD_CS + kk];
                const double bb = ij == 0 ? ych[kk] : 0.0;
                racc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bb, racc, 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // ---- G (column-scaled handle: S G_V S, r = S r_V) into M, r into rv ----
    auto sc = [&](int k) { return (scale && live && k < nb) ? scale[(size_t)b * nb + k] : 1.0; };
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
        if (has[q]) {
            const int j = 16 * tj[q] + ij;
            const double sj = sc(j);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 16 * ti[q] + kq + 4 * r;
                const double v = scale ? acc[q][r] * (sc(i) * sj) : acc[q][r];
                M[i * S64_LS + j] = v;
                if (PIVOT) M[j * S64_LS + i] = v;
            }
        }
    }
    if (rtile && ij == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = 16 * wg + kq + 4 * r;
            rv[i] = racc[r] * sc(i);
            if (r_out && live && i < nb) r_out[(size_t)b * nb + i] = rv[i];
        }
    }
    if (gt == 0) misc_i[1] = 0;
    __syncthreads();
    double dsum = 0.0;
    if (delta) {                       // sum(dtd_b) in index order, every thread its own copy (LDS broadcast reads)
        for (int k = 0; k < nb; ++k) dsum += M[k * S64_LS + k];
        __syncthreads();
    }
    if (gt < ncp) {
        if (!live || gt >= nb) M[gt * S64_LS + gt] = 1.0;                          // padding: identity
        else {
            const double d = M[gt * S64_LS + gt];
            if (diag_out) diag_out[(size_t)b * nb + gt] = d;
            if (damp) M[gt * S64_LS + gt] = d + damp[(size_t)b * nb + gt];
            else if (delta) {
                const double mean = dsum / nb;
                const double lo = BD_MIN_DIAGONAL * mean, hi = BD_MAX_DIAGONAL * mean;
                const double dc = d > hi ? hi : (d < lo ? lo : d);
                M[gt * S64_LS + gt] = d + dc * (1.0 / delta[b]);
            }
        }
    }
    __syncthreads();

    if (!PIVOT) {
        // ---- dense_cholesky.jl:43-59: G + D = U'U, unpivoted (the blocked scheme of s64_chol on NT tile rows) ----
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
        const int fail = misc_i[1];
        if (wg == 0 && live) {
            if (binfo && lane == 0) binfo[b] = fail;
            if (fail) {
                if (lane == 0 && !binfo) {
                    atomicMin(&info[0], b * nb + fail);
                    atomicMin(&info[1], b);
                }
            } else {
                // U'z = r, U x = z: one wavefront, lane = unknown, the pivot row / column broadcast with v_readlane
                const bool in = lane < ncp;
                const int li = in ? lane : 0;
                const double dinv = 1.0 / M[li * S64_LS + li];
                double z = in ? rv[li] : 0.0;
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
                if (lane < nb) x[(size_t)b * nb + lane] = z;
            }
        }
    } else {
        // ---- dense_cholesky.jl:29-35: cholesky!(Symmetric(J'J), Val(true)), tol = 0: dpstf2 on the full symmetric G_b in
        // LDS, one column per step, the right-hand side carried along as the forward solve; factor rows into W ----
        int dead = 0, rank = nb;
        double rz = lane < nb ? rv[lane] : 0.0;    // (wavefront 0 of the group) permuted right-hand side -> z
        int pm = lane;                             // ... and the permutation
        for (int j = 0; j < nb; ++j) {
            if (wg == 0) {
                double d = (lane >= j && lane < nb) ? M[lane * S64_LS + lane] : -INFINITY;
                int idx = lane;
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) {
                    const double od = __shfl_xor(d, off);
                    const int oi = __shfl_xor(idx, off);
                    if (od > d || (od == d && oi < idx)) { d = od; idx = oi; }
                }
                if (lane == 0) { misc_i[0] = idx; misc_d[0] = d; }
            }
            __syncthreads();
            const int p = __builtin_amdgcn_readfirstlane(misc_i[0]);
            const double ajj = misc_d[0];
            if (!dead && !(ajj > 0.0)) { dead = 1; rank = j; }
            if (!dead && p != j) {                 // P'GP: rows and columns j <-> p
                if (gt < nb && gt != j && gt != p) {
                    double t = M[j * S64_LS + gt]; M[j * S64_LS + gt] = M[p * S64_LS + gt]; M[p * S64_LS + gt] = t;
                    t = M[gt * S64_LS + j]; M[gt * S64_LS + j] = M[gt * S64_LS + p]; M[gt * S64_LS + p] = t;
                }
                if (gt == j) {
                    const double t = M[j * S64_LS + j]; M[j * S64_LS + j] = M[p * S64_LS + p]; M[p * S64_LS + p] = t;
                }
                if (gt < j) {                      // ... and the columns of the factor rows that are already final
                    const double t = W[gt * S64_LS + j]; W[gt * S64_LS + j] = W[gt * S64_LS + p]; W[gt * S64_LS + p] = t;
                }
                if (wg == 0) {
                    const double vj = s64_readlane(rz, j), vp = s64_readlane(rz, p);
                    const int qj = __builtin_amdgcn_readlane(pm, j), qp = __builtin_amdgcn_readlane(pm, p);
                    if (lane == j) { rz = vp; pm = qp; }
                    if (lane == p) { rz = vj; pm = qj; }
                }
            }
            __syncthreads();
            if (!dead) {
                const double d = sqrt(ajj);
                const bool right = lane > j && lane < nb;
                const double u = right ? M[j * S64_LS + lane] / d : 0.0;     // row j of U, every wavefront its own copy
                if (wg == 0) {
                    if (lane < nb) W[j * S64_LS + lane] = lane == j ? d : u;
                    const double zj = s64_readlane(rz / d, j);
                    if (lane == j) rz = zj;
                    else if (right) rz -= u * zj;
                }
                for (int i = j + 1 + wg; i < nb; i += G) {
                    const double ui = s64_readlane(u, __builtin_amdgcn_readfirstlane(i));
                    if (right) M[i * S64_LS + lane] -= ui * u;
                }
            }
            __syncthreads();
        }
        if (wg == 0 && live) {
            if (binfo && lane == 0) binfo[b] = dead ? nb - rank : 0;
            if (dead) {
                if (lane == 0 && !binfo) {
                    atomicMin(&info[1], b);
                    atomicAdd(&info[2], nb - rank);
                }
            } else {
                const bool in = lane < nb;
                const int li = in ? lane : 0;
                const double dinv = 1.0 / W[li * S64_LS + li];
                for (int k = nb - 1; k >= 0; --k) {
                    const double u = W[li * S64_LS + k];
                    const double xk = s64_readlane(rz * dinv, k);
                    if (lane == k) rz = xk;
                    else if (lane < k) rz -= u * xk;
                }
                if (in) x[(size_t)b * nb + pm] = rz;      // invpermute!
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
extern "C" int lsq_blockdiag_create(lsq_ctx *c, int nblocks, int mb, int nb, lsq_mat **out) {
    LSQ_RANGE("lsq_blockdiag_create");
    if (!c || !out) { lsq_set_error("lsq_blockdiag_create: null argument"); return LSQ_EARG; }
    if (nblocks < 1 || mb < 1 || nb < 1) {
        lsq_set_error("lsq_blockdiag_create: needs nblocks >= 1, mb >= 1, nb >= 1 (got %d, %d, %d)", nblocks, mb, nb);
        return LSQ_EDIM;
    }
    const long long m = (long long)nblocks * mb, n = (long long)nblocks * nb, nnz = m * nb;
    if (m > INT_MAX || n > INT_MAX || nnz > 2147483000LL) {
        lsq_set_error("lsq_blockdiag_create: %d blocks of %d x %d do not fit 32-bit indices", nblocks, mb, nb);
        return LSQ_EDIM;
    }
    try {
        std::vector<int> colptr((size_t)n + 1), rowval((size_t)nnz);
        for (long long j = 0; j <= n; ++j) colptr[(size_t)j] = (int)(j * mb);
        for (int b = 0; b < nblocks; ++b)
            for (int j = 0; j < nb; ++j) {
                int *rv = rowval.data() + ((size_t)b * nb + j) * mb;
                for (int i = 0; i < mb; ++i) rv[i] = b * mb + i;
            }
        LSQ_TRY(lsq_csc_create(c, (int)m, (int)n, colptr.data(), rowval.data(), out));
    } catch (const std::bad_alloc &) {
        lsq_set_error("lsq_blockdiag_create: out of host memory while building the pattern");
        return LSQ_EHIP;
    }
    (*out)->bd_blocks = nblocks;
    (*out)->bd_mb = mb;
    (*out)->bd_nb = nb;
    return LSQ_OK;
}

extern "C" int lsq_mat_blockdiag_info(const lsq_mat *J, int *nblocks, int *mb, int *nb) {
    if (!J) { lsq_set_error("lsq_mat_blockdiag_info: null argument"); return LSQ_EARG; }
    if (nblocks) *nblocks = J->bd_blocks;
    if (mb) *mb = J->bd_mb;
    if (nb) *nb = J->bd_nb;
    return LSQ_OK;
}

extern "C" int lsq_solver_blockdiag_path(const lsq_solver *s, int *path, int *block) {
    if (!s) { lsq_set_error("lsq_solver_blockdiag_path: null argument"); return LSQ_EARG; }
    if (path) *path = s->last_bd_path;
    if (block) *block = s->last_bd_block;
    return LSQ_OK;
}

int lsq_blockdiag_solver_alloc(lsq_solver *s, const lsq_mat *J) {
    if (J->bd_nb > 64) {
        lsq_set_error("Cholesky() on a block-diagonal Jacobian needs blocks of at most 64 columns (got nb = %d): one block's "
                      "normal matrix must fit the 64 x 64 in-LDS factorisation. Use LSMR()", J->bd_nb);
        return LSQ_EARG;
    }
    s->bd_blocks = J->bd_blocks;
    s->bd_mb = J->bd_mb;
    s->bd_nb = J->bd_nb;
    LSQ_HIP(hipMalloc(&s->d_info, 4 * sizeof(int)));       // (the factors never leave LDS: nothing else to allocate)
    return LSQ_OK;
}

struct BdExtra {       // the batched loop's operands of k_bd_solve (all null: the plain solve)
    const int *active = nullptr;
    int *binfo = nullptr;
    double *r_out = nullptr, *diag_out = nullptr;
    const double *delta = nullptr;
};

template <int G, bool PIVOT>
static int bd_launch(lsq_ctx *c, lsq_mat *J, const double *d_y, const double *d_damp, double *d_x, int *d_info, const BdExtra &e) {
    const int B = J->bd_blocks;
    const size_t lds = (G == 4 ? 1 : 4) * bd_group_doubles(J->bd_nb) * sizeof(double);
    LSQ_TRY(lsq_set_lds(c, (const void *)k_bd_solve<G, PIVOT>, lds));
    const int grid = G == 4 ? B : (B + 3) / 4;
    LSQ_LAUNCH((k_bd_solve<G, PIVOT>), dim3(grid), dim3(256), lds, c->stream, B, J->bd_mb, J->bd_nb,
               (const double *)J->csc.d_val, J->d_colscale, d_y, d_damp, d_x, d_info, e.active, e.binfo, e.r_out, e.diag_out,
               e.delta);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

// One batched solve for the per-block trust-region loop (lsq_batched.hip): pivot = false: LM, damping formed in the kernel
// from d_delta (B trust-region radii); pivot = true: Dogleg's Gauss-Newton step.  Only blocks with d_active[b] != 0 are
// solved (x_b, r_b, diag_b, binfo[b] of the others are left alone).  Nothing is read back.
int lsq_blockdiag_solve_blocks(lsq_ctx *c, lsq_mat *J, bool pivot, const double *d_y, const double *d_delta, double *d_x,
                               const int *d_active, int *d_binfo, double *d_r, double *d_diag) {
    LSQ_TRY(lsq_ensure_csc(J));
    BdExtra e;
    e.active = d_active; e.binfo = d_binfo; e.r_out = d_r; e.diag_out = d_diag; e.delta = pivot ? nullptr : d_delta;
    const bool wide = J->bd_nb > 16;
    if (pivot) return wide ? bd_launch<4, true>(c, J, d_y, nullptr, d_x, nullptr, e) : bd_launch<1, true>(c, J, d_y, nullptr, d_x, nullptr, e);
    return wide ? bd_launch<4, false>(c, J, d_y, nullptr, d_x, nullptr, e) : bd_launch<1, false>(c, J, d_y, nullptr, d_x, nullptr, e);
}

// dense_cholesky.jl:29-35 (d_damp == nullptr: pivoted, Dogleg) and :43-59 (damped, unpivoted, LM) on the stacked system
int lsq_blockdiag_solve(lsq_solver *s, lsq_mat *J, const double *d_y, const double *d_damp, double *d_x, int *nmul) {
    lsq_ctx *c = s->ctx;
    if (J->kind != LSQ_MAT_CSC || J->bd_blocks != s->bd_blocks || J->bd_mb != s->bd_mb || J->bd_nb != s->bd_nb ||
        J->m != s->m || J->n != s->n) {
        lsq_set_error("cholesky: this solver was allocated for a block-diagonal Jacobian of %d blocks of %d x %d",
                      s->bd_blocks, s->bd_mb, s->bd_nb);
        return LSQ_EDIM;
    }
    LSQ_TRY(lsq_ensure_csc(J));        // (a device-side g! may have written the product mirrors only)
    LSQ_LAUNCH(k_bd_init, dim3(1), dim3(64), 0, c->stream, s->d_info);
    const bool wide = s->bd_nb > 16;
    const BdExtra none;
    if (d_damp) LSQ_TRY(wide ? (bd_launch<4, false>(c, J, d_y, d_damp, d_x, s->d_info, none)) : (bd_launch<1, false>(c, J, d_y, d_damp, d_x, s->d_info, none)));
    else LSQ_TRY(wide ? (bd_launch<4, true>(c, J, d_y, d_damp, d_x, s->d_info, none)) : (bd_launch<1, true>(c, J, d_y, d_damp, d_x, s->d_info, none)));
    s->last_bd_path = d_damp ? 1 : 2;
    s->last_bd_block = -1;
    int st4[4] = {0, 0, 0, 0};
    LSQ_TRY(lsq_read_ints(c, s->d_info, s->d_info + 1, s->d_info + 2, nullptr, st4));
    if (nmul) *nmul = 1;
    if (st4[1] != INT_MAX) {
        s->last_bd_block = st4[1];
        if (d_damp) {
            lsq_set_error("PosDefException: matrix is not positive definite; Cholesky failed at %d", st4[0]);
            return LSQ_ENOTPD;
        }
        lsq_set_error("RankDeficientException(%d)", s->n - st4[2]);
        return LSQ_ERANK;
    }
    return LSQ_OK;
}
