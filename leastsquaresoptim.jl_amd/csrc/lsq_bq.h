// The pieces of the streaming block Householder step (the triangle-over-rectangle step of TSQR) that k_bq_solve
// (lsq_blockqr.hip) and the bordered elimination (lsq_borderedqr.hip) share: the barrier of a block's thread group, the
// quad sum and dlarfg.
#pragma once
#include "lsq_common.h"

#ifdef __HIPCC__
template <int G>
__device__ __forceinline__ void bq_sync() {
    if (G == 4) __syncthreads();
    else {      // one wavefront owns the block: order its own LDS traffic, nothing to wait for
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
}

__device__ __forceinline__ double bq_quad_sum(double v) {   // (p0 + p1) + (p2 + p3), the same bits in the four threads
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    return v;
}

// dlarfg on (alpha, x) with |x|^2 = s2: H = I - tau v v', v = (1, x * sc), H (alpha, x) = (beta, 0).  s2 is a plain sum of
// squares (as in k_qrcp_solve), without dnrm2's scaling and dlarfg's safmin loop: columns whose entries leave about
// 1e-150 .. 1e150 overflow or underflow here where LAPACK would not.
__device__ __forceinline__ void bq_larfg(double alpha, double s2, double *tau, double *sc, double *beta) {
    if (s2 == 0.0) { *tau = 0.0; *sc = 0.0; *beta = alpha; return; }
    const double bt = -copysign(hypot(alpha, sqrt(s2)), alpha);
    *tau = (bt - alpha) / bt;
    *sc = 1.0 / (alpha - bt);
    *beta = bt;
}
#endif
