// Covariance pieces shared by k_bd_cov (lsq_cov.hip) and k_bb_cov_schur / k_bb_cov_back (lsq_bordered.hip): from an upper
// triangular factor U (G = U'U) in LDS to Cov = inv(G) = inv(U) inv(U)', on NT = ceil(n / 16) tile rows, operands and layouts
// as in lsq_small64.h.  What is kept is Y = inv(U)' (block LOWER triangular), because that is what s64_chol16 leaves in its
// identity lanes for the diagonal blocks; Cov = Y'Y.  G wavefronts work on one matrix (wg = this one's index); the routines
// with barriers must be called by every wavefront of the WORKGROUP.
#pragma once
#include "lsq_small64.h"

// Y_kk = inv(U_kk)' for the NT diagonal blocks of an upper triangular U by back substitution, one lane per column (the
// scheme of s64_diaginv_upper, stored transposed; zeros above the diagonal inside the block).  No barrier.
template <int G>
__device__ __forceinline__ void cov_diaginv_t(const double *__restrict__ U, double *__restrict__ Y, int NT, int wg, int lane) {
    for (int kb = wg; kb < NT; kb += G) {
        if (lane < 16) {
            const int o = 16 * kb, cc = lane;
            double x[16];
#pragma unroll
            for (int r = 15; r >= 0; --r) {
                double acc = r == cc ? 1.0 : 0.0;
#pragma unroll
                for (int k = r + 1; k < 16; ++k) acc -= U[(o + r) * S64_LS + o + k] * x[k];
                x[r] = r <= cc ? acc * s64_rcp(U[(o + r) * S64_LS + o + r]) : 0.0;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) Y[(o + cc) * S64_LS + o + r] = x[r];
        }
    }
}

// Y <- inv(U)' below the diagonal blocks, which already hold inv(U_kk)': with L = U', Y L = I gives
//     Y_ji = -(sum_{k = i+1 .. j} Y_jk U_ik') Y_ii      (j > i),
// tile (j, i) needs tiles (j, k) with j - k < j - i only, so the tiles of one distance d = j - i are independent: NT - 1
// levels, a workgroup barrier behind each (none for NT = 1).  The sum is formed TRANSPOSED, P' = sum U_ik Y_jk': an MFMA
// accumulator holds D[(l >> 4) + 4 r][l & 15], which read as P[l & 15][(l >> 4) + 4 r] is the A operand of the second
// product with k running over (l >> 4) + 4 r -- no trip through LDS between the two.
template <int G>
__device__ __forceinline__ void cov_inv_levels(const double *__restrict__ U, double *__restrict__ Y, int NT, int wg, int lane) {
    const int ij = lane & 15, kq = lane >> 4;
    for (int d = 1; d < NT; ++d) {
        for (int i = wg; i + d < NT; i += G) {
            const int j = i + d;
            s64_v4d p = {0.0, 0.0, 0.0, 0.0};
            for (int k = i + 1; k <= j; ++k) s64_tile_mma<false, true>(p, U, 16 * i, 16 * k, Y, 16 * j, 16 * k, 1, lane);
            s64_v4d a = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int r = 0; r < 4; ++r)
                a = __builtin_amdgcn_mfma_f64_16x16x4f64(p[r], Y[(16 * i + kq + 4 * r) * S64_LS + 16 * i + ij], a, 0, 0, 0);
            s64_tile_store<false>(Y, 16 * j, 16 * i, a, -1.0, lane);
        }
        __syncthreads();
    }
}

// tile (ti, tj), ti <= tj, of Y'P for a block lower triangular Y and a P whose tiles (kt, tj) with kt < tj do not
// contribute (P = Y: Cov = Y'Y)
__device__ __forceinline__ s64_v4d cov_tile(const double *__restrict__ Y, const double *__restrict__ P, int NT, int ti, int tj,
                                            int lane) {
    s64_v4d a = {0.0, 0.0, 0.0, 0.0};
    for (int kt = tj; kt < NT; ++kt) s64_tile_mma<true, false>(a, Y, 16 * kt, 16 * ti, P, 16 * kt, 16 * tj, 1, lane);
    return a;
}

// accumulator tile (ti, tj), ti <= tj, times s2 -> the n x n row-major matrix `cov` in global memory (entries (i, j) and
// (j, i) from the same register: both triangles carry the same bits) and sqrt of the diagonal -> `se`; either may be null
__device__ __forceinline__ void cov_store(double *__restrict__ cov, double *__restrict__ se, int n, int ti, int tj,
                                          const s64_v4d &a, double s2, int lane) {
    const int j = 16 * tj + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = 16 * ti + (lane >> 4) + 4 * r;
        if (i <= j && j < n) {
            const double v = s2 * a[r];
            if (cov) {
                cov[(size_t)i * n + j] = v;
                cov[(size_t)j * n + i] = v;
            }
            if (se && i == j) se[i] = sqrt(v);
        }
    }
}
