// BorderedQR() on a bordered block-diagonal Jacobian J = [blkdiag(J_1 .. J_B) | C] (lsq_blockdiag_bordered_create) with nb <= 64,
// any ng >= 1: LevenbergMarquardt's damped solve as the least-squares problem it is,
//     min || [J S; diag(sqrt(damp))] x - [y; 0] ||_2        (S: the handle's column scale, if one is set)
// by Householder reflectors.  Neither J'J nor any part of it is formed, so the solve pays cond(J) where Cholesky() and Schur()
// on this handle pay cond(J)^2.  The locals are not pivoted: Householder QR is columnwise backward stable without it.
//
// Per block b the rows of [J_b | C_b | y_b] are eliminated against a running triangle that starts as diag(sqrt(damp_b)) -- it
// is upper triangular already, so the damping of the locals costs no extra rows:
//     Q_b' [diag(sqrt(damp_b)) 0 0; J_b C_b y_b] = [R_b W_b z_b; 0 F_b r_b]
// The stack of the F_b ((B mb) x ng, the shape of C) with right-hand side r and the last ng damping values is the problem of the
// shared unknowns: x_g from a dense QR() solver this one owns; then x_b = inv(R_b) (z_b - W_b x_g).  Stream order:
//   k_bdq_factor<G, H>  per block, the geometry and the triangle-over-rectangle step of k_bq_solve (16 < nb <= 64: one
//                     workgroup per block; nb <= 16: one wavefront per block, four per workgroup): chunks of H rows of J_b
//                     against R_b, y_b carried as column nb.  Writes R_b, z_b, r_b, and per chunk the reflector vectors
//                     (the place of the chunk in a copy of the block values) and their nb taus.
//   k_bdq_apply<H>    per (block, tile of 64 border columns): replays the reflectors on the tile, one quad of threads per
//                     column -- a column needs nothing from its neighbours, so the only barriers are those of the chunk
//                     staging.  Writes the tile of W_b and of F_b.  LDS does not depend on ng or mb.
//   inner solver      a dense LSQ_QR lsq_solver (for_lm) with m = B mb, n = ng (lsq_solver::inner) on a dense handle that
//                     wraps F (lsq_solver::inner_J): one lsq_qr_solve with every path and retry it has.
//   k_bdq_back        one workgroup per block: x_b = inv(R_b) (z_b - W_b x_g).
// The factorisation of the locals is split from its application to the border because global fits often have far fewer
// blocks than the chip has CUs: the reflectors of a block are B-way parallel, their application B ceil(ng / 64)-way.
// No floating-point atomics, no workgroup waits for another, every sum has a fixed association: two runs give identical bits
// (outside whatever the inner QR() does on its own).
//
// A diagonal entry of some R_b that is exactly zero or not finite (possible only where a damping value is zero or an operand
// is not finite) is LSQ_ERANK with the 1-based stacked column b nb + k, the lowest one.  Dogleg is not offered, for the reason
// lsq_bordered.hip gives for Dogleg(Cholesky()).
#include <cfloat>
#include <climits>

#include "lsq_solver.h"
#include "lsq_bq.h"

int lsq_bordered_refuse_dogleg();                                                       // lsq_bordered.hip

constexpr int BDQ_TW = 64;         // border columns per tile: one per quad of the 256 threads

// doubles of LDS per block of k_bdq_factor: R with y's column nb (column stride nb | 1) | chunk (nb + 1 columns of H + 1)
// | tau | sc (the reflectors of the chunk at hand)
__host__ __device__ static inline size_t bdq_factor_doubles(int nb, int H) {
    return (size_t)(nb | 1) * (nb + 1) + (size_t)(nb + 1) * (H + 1) + 2 * (size_t)nb;
}
// ... of k_bdq_apply: W tile (64 columns of nb | 1) | reflector chunk (nb columns of H + 1) | border chunk (64 of H + 1) | tau
static inline size_t bdq_apply_doubles(int nb, int H) {
    return (size_t)BDQ_TW * (nb | 1) + (size_t)(nb + BDQ_TW) * (H + 1) + (size_t)nb;
}

__global__ void k_bdq_init(int *info) {
    if (threadIdx.x == 0) info[0] = INT_MAX;
}

// info[0]: the lowest failing stacked column (atomicMin); info[1 + b]: block b's first failing column (1-based) or 0.
// V: the reflector vectors, laid out like the block values; T: nb taus per (block, chunk).
template <int G, int H>
__global__ void __launch_bounds__(256)
k_bdq_factor(int B, int mb, int nb, const double *__restrict__ vals, const double *__restrict__ scale,
             const double *__restrict__ y, const double *__restrict__ damp, double *__restrict__ Rout,
             double *__restrict__ zout, double *__restrict__ rout, double *__restrict__ V, double *__restrict__ T,
             int *__restrict__ info) {
    extern __shared__ double bdq_lds[];
    constexpr int GT = 64 * G, HQ = H / 4, CS = H + 1, CP = GT / H;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int gt = G == 4 ? tid : lane;                                  // thread inside its group
    const int b = G == 4 ? (int)blockIdx.x : (int)blockIdx.x * 4 + wv;
    if (b >= B) return;                // (G == 1: the wavefronts of a workgroup never meet at a barrier)
    const int ls = nb | 1;
    double *R = bdq_lds + (G == 4 ? 0 : wv) * bdq_factor_doubles(nb, H);
    double *ch = R + ls * (nb + 1);
    double *tauv = ch + (nb + 1) * CS, *scv = tauv + nb;
    const int qi = gt >> 2, q = gt & 3;                    // quad, thread inside it
    const size_t vbase = (size_t)b * mb * nb, ybase = (size_t)b * mb, xbase = (size_t)b * nb;
    const int nch = (mb + H - 1) / H;

    for (int e = gt; e < ls * (nb + 1); e += GT) R[e] = 0.0;
    bq_sync<G>();
    if (gt < nb) R[gt * ls + gt] = sqrt(damp[xbase + gt]);          // the damping rows ARE the first triangle

    const int lr = gt & (H - 1), c0 = gt / H;
    double reg[HQ], yreg = 0.0;
    auto load = [&](int row0) {
        const int row = row0 + lr;
        const bool ok = row < mb;
#pragma unroll
        for (int p = 0; p < HQ; ++p) {
            const int c = c0 + p * CP;
            reg[p] = (ok && c < nb) ? vals[vbase + (size_t)c * mb + row] : 0.0;
        }
        if (gt < H) yreg = ok ? y[ybase + row] : 0.0;
    };
    load(0);
    for (int c = 0; c < nch; ++c) {
#pragma unroll
        for (int p = 0; p < HQ; ++p) {
            const int col = c0 + p * CP;
            if (col < nb) ch[col * CS + lr] = scale ? reg[p] * scale[xbase + col] : reg[p];   // column-scaled handle: J_b S_b
        }
        if (gt < H) ch[nb * CS + gt] = yreg;
        bq_sync<G>();
        if (c + 1 < nch) load((c + 1) * H);                // in flight during the elimination
        // the chunk (H rows x (nb + 1) columns, staged as [column][row]) against R: nb reflectors.  Step j leaves column j
        // of the chunk as it found it: with scv[j] it is the reflector's vector
        for (int j = 0; j < nb; ++j) {
            double v[HQ], s2 = 0.0;
#pragma unroll
            for (int t = 0; t < HQ; ++t) { v[t] = ch[j * CS + q + 4 * t]; s2 += v[t] * v[t]; }
            s2 = bq_quad_sum(s2);
            double tau, sc, beta;
            bq_larfg(R[j * ls + j], s2, &tau, &sc, &beta);
            const int k = j + 1 + qi;                      // this quad's column (k == nb: the right-hand side)
            const bool on = tau != 0.0 && k <= nb;
            double a[HQ], dot = 0.0;
#pragma unroll
            for (int t = 0; t < HQ; ++t) {
                v[t] *= sc;
                a[t] = on ? ch[k * CS + q + 4 * t] : 0.0;
                dot += v[t] * a[t];
            }
            dot = bq_quad_sum(dot);
            if (on) {
                const double rjk = R[k * ls + j];
                const double tw = tau * (dot + rjk);
#pragma unroll
                for (int t = 0; t < HQ; ++t) ch[k * CS + q + 4 * t] = a[t] - v[t] * tw;
                if (q == 0) R[k * ls + j] = rjk - tw;
            }
            if (gt == 0) { tauv[j] = tau; scv[j] = sc; }
            bq_sync<G>();
            if (gt == 0) R[j * ls + j] = beta;             // (read as alpha by every thread in front of the barrier)
        }
        // the chunk's reflectors and its rows of r_b = (Q_b'[0; y_b]) below the triangle
        const int row = c * H + lr;
#pragma unroll
        for (int p = 0; p < HQ; ++p) {
            const int col = c0 + p * CP;
            if (col < nb && row < mb) V[vbase + (size_t)col * mb + row] = ch[col * CS + lr] * scv[col];
        }
        if (gt < H && c * H + gt < mb) rout[ybase + c * H + gt] = ch[nb * CS + gt];
        if (gt < nb) T[((size_t)b * nch + c) * nb + gt] = tauv[gt];
        bq_sync<G>();                                      // the next chunk is staged over this one
    }
    bq_sync<G>();
    if (gt == 0) {
        int fail = 0;
        for (int k = 0; k < nb && !fail; ++k) {
            const double d = fabs(R[k * ls + k]);
            if (!(d > 0.0 && d <= DBL_MAX)) fail = k + 1;
        }
        info[1 + b] = fail;
        if (fail) atomicMin(&info[0], b * nb + fail);
    }
    double *rb = Rout + (size_t)b * nb * nb;
    for (int e = gt; e < nb * nb; e += GT) {               // rows of R_b, zeros below the diagonal
        const int k = e / nb, c = e - k * nb;
        rb[e] = c >= k ? R[c * ls + k] : 0.0;
    }
    if (gt < nb) zout[xbase + gt] = R[nb * ls + gt];
}

// Block b = blockIdx.x, border columns 64 blockIdx.y ..: the reflectors of k_bdq_factor, chunk by chunk in its order, on
// [W; C_b[:, tile]] with W = 0 at the start (the damping rows have no entries in the border).  Thread = (column qi, rows
// q (mod 4) of the chunk); the column's chunk lives in registers across the nb reflectors.  A block that failed stores zeros:
// what follows in the stream works on finite numbers, and the solve reports the block's column whatever they give.
template <int H>
__global__ void __launch_bounds__(256)
k_bdq_apply(int B, int mb, int nb, int ng, const double *__restrict__ vals, const double *__restrict__ scale,
            const double *__restrict__ V, const double *__restrict__ T, const int *__restrict__ info,
            double *__restrict__ Wout, double *__restrict__ F) {
    extern __shared__ double bdq_lds[];
    constexpr int HQ = H / 4, CS = H + 1, CP = 256 / H;
    const int tid = threadIdx.x, qi = tid >> 2, q = tid & 3;
    const int b = blockIdx.x, col0 = BDQ_TW * (int)blockIdx.y;
    const int ls = nb | 1;
    double *Wt = bdq_lds;                                  // [column][row of the triangle]
    double *vs = Wt + BDQ_TW * ls;                         // reflector vectors of the chunk: [reflector][row]
    double *cc = vs + nb * CS;                             // the border tile's chunk: [column][row]
    double *tv = cc + BDQ_TW * CS;
    const size_t m = (size_t)B * mb;
    const size_t vbase = (size_t)b * mb * nb, cbase = m * nb + (size_t)b * mb, fbase = (size_t)b * mb;
    const size_t ldw = (size_t)B * nb;
    const int nch = (mb + H - 1) / H;
    const bool fail = info[1 + b] != 0;

    for (int e = tid; e < BDQ_TW * ls; e += 256) Wt[e] = 0.0;
    const int lr = tid & (H - 1), c0 = tid / H;
    double vreg[HQ], creg[HQ];                             // 64 columns in HQ passes of CP columns
    auto load = [&](int row0) {
        const int row = row0 + lr;
        const bool ok = row < mb;
#pragma unroll
        for (int p = 0; p < HQ; ++p) {
            const int c = c0 + p * CP, gc = col0 + c;
            vreg[p] = (ok && c < nb) ? V[vbase + (size_t)c * mb + row] : 0.0;
            double v = (ok && gc < ng) ? vals[cbase + (size_t)gc * m + row] : 0.0;
            if (scale && gc < ng) v *= scale[ldw + gc];    // column-scaled handle: C S_g
            creg[p] = v;
        }
    };
    load(0);
    for (int c = 0; c < nch; ++c) {
#pragma unroll
        for (int p = 0; p < HQ; ++p) {
            const int col = c0 + p * CP;
            if (col < nb) vs[col * CS + lr] = vreg[p];
            cc[col * CS + lr] = creg[p];
        }
        if (tid < nb) tv[tid] = T[((size_t)b * nch + c) * nb + tid];
        __syncthreads();
        if (c + 1 < nch) load((c + 1) * H);                // in flight during the reflectors
        double a[HQ];
#pragma unroll
        for (int t = 0; t < HQ; ++t) a[t] = cc[qi * CS + q + 4 * t];
        for (int j = 0; j < nb; ++j) {
            const double tau = tv[j];
            if (tau == 0.0) continue;                      // (the same in every thread)
            double dot = 0.0;
#pragma unroll
            for (int t = 0; t < HQ; ++t) dot += vs[j * CS + q + 4 * t] * a[t];
            dot = bq_quad_sum(dot);
            const double rjk = Wt[qi * ls + j];
            const double tw = tau * (dot + rjk);
#pragma unroll
            for (int t = 0; t < HQ; ++t) a[t] = a[t] - vs[j * CS + q + 4 * t] * tw;
            if (q == 0) Wt[qi * ls + j] = rjk - tw;        // (read again by this quad only, behind the next chunk's barrier)
        }
#pragma unroll
        for (int t = 0; t < HQ; ++t) cc[qi * CS + q + 4 * t] = a[t];
        __syncthreads();
        const int row = c * H + lr;
#pragma unroll
        for (int p = 0; p < HQ; ++p) {                     // the chunk's rows of F_b, down the columns of the stack
            const int col = c0 + p * CP, gc = col0 + col;
            if (row < mb && gc < ng) F[(size_t)gc * m + fbase + row] = fail ? 0.0 : cc[col * CS + lr];
        }
        __syncthreads();                                   // the next chunk is staged over this one
    }
    __syncthreads();
    const int ncol = ng - col0 < BDQ_TW ? ng - col0 : BDQ_TW;
    for (int e = tid; e < ncol * nb; e += 256) {
        const int j = e / nb, i = e - j * nb;
        Wout[(size_t)(col0 + j) * ldw + (size_t)b * nb + i] = fail ? 0.0 : Wt[j * ls + i];
    }
}

// x_b = inv(R_b) (z_b - W_b x_g): one workgroup per block.  The product W_b x_g: thread = (row i, column class jj), the thread
// sums the columns j = jj, jj + cpl, .. (cpl = 256 / nb classes) in ascending order; the first wavefront subtracts the classes
// in index order and substitutes back (lane = unknown, the pivot row broadcast with v_readlane).
__global__ void __launch_bounds__(256)
k_bdq_back(int B, int nb, int ng, const double *__restrict__ Rin, const double *__restrict__ zin, const double *__restrict__ Wst,
           const double *__restrict__ xg, double *__restrict__ x) {
    extern __shared__ double bdq_lds[];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int ld = nb | 1;
    double *sR = bdq_lds;
    double *sp = sR + nb * ld;                         // 256
    const double *rb = Rin + (size_t)b * nb * nb;
    for (int e = tid; e < nb * nb; e += 256) {
        const int k = e / nb, c = e - k * nb;
        sR[k * ld + c] = rb[e];
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
    const double dinv = 1.0 / sR[li * ld + li];
    for (int k = nb - 1; k >= 0; --k) {
        const double u = sR[li * ld + k];
        const double xk = lsq_readlane_f64(t * dinv, k);
        if (lane == k) t = xk;
        else if (lane < k) t -= u * xk;
    }
    if (in) x[(size_t)b * nb + lane] = t;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
struct BdqLayout {
    int H, nch;
    size_t R, z, W, V, T, F, r, total;             // offsets into d_work (doubles)
};
// The chunk height is the launch-time choice of BlockQR(): 64 rows when a block has more than 32, else 32; both kernels use it
static BdqLayout bdq_layout(int B, int mb, int nb, int ng) {
    BdqLayout l;
    l.H = mb > 32 ? 64 : 32;
    l.nch = (mb + l.H - 1) / l.H;
    const size_t Bn = (size_t)B * nb, m = (size_t)B * mb;
    l.R = 0;
    l.z = l.R + Bn * nb;
    l.W = l.z + Bn;
    l.V = l.W + Bn * ng;
    l.T = l.V + m * nb;
    l.F = l.T + (size_t)B * l.nch * nb;
    l.r = l.F + m * ng;
    l.total = l.r + m;
    return l;
}

int lsq_borderedqr_solver_alloc(lsq_solver *s, const lsq_mat *J) {
    if (J->kind != LSQ_MAT_CSC || J->br_blocks < 1) {
        const char *what = J->kind == LSQ_MAT_DENSE ? "a dense handle (lsq_dense_create): use QR()"
                           : J->kind != LSQ_MAT_CSC ? "an operator handle (lsq_op_create): use LSMR()"
                           : J->bd_blocks > 0       ? "a block-diagonal handle without shared columns (lsq_blockdiag_create): "
                                                      "use BlockQR()"
                                                    : "a plain CSC handle (lsq_csc_create): use LSMR()";
        lsq_set_error("BorderedQR() needs a bordered block-diagonal Jacobian (lsq_blockdiag_bordered_create); this is %s", what);
        return LSQ_EARG;
    }
    if (J->br_nb > 64) {
        lsq_set_error("BorderedQR() on a bordered block-diagonal Jacobian needs nb <= 64 (got nb = %d, ng = %d): one block's "
                      "triangular factor must fit the in-LDS elimination. Use LSMR()", J->br_nb, J->br_ng);
        return LSQ_EARG;
    }
    if (!s->for_lm) return lsq_bordered_refuse_dogleg();
    lsq_ctx *c = s->ctx;
    s->br_blocks = J->br_blocks;
    s->br_mb = J->br_mb;
    s->br_nb = J->br_nb;
    s->br_ng = J->br_ng;
    const BdqLayout l = bdq_layout(J->br_blocks, J->br_mb, J->br_nb, J->br_ng);
    s->work_elems = l.total;
    LSQ_HIP(hipMalloc(&s->d_work, s->work_elems * sizeof(double)));
    LSQ_HIP(hipMalloc(&s->d_info, ((size_t)J->br_blocks + 1) * sizeof(int)));
    lsq_solver *in = new lsq_solver();     // the dense QR() solver of the shared unknowns: (m + ng) ng doubles
    in->ctx = c;
    in->kind = LSQ_QR;
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
    lsq_mat *Fm = new lsq_mat();           // F as a dense handle: a view into d_work, it owns nothing
    Fm->ctx = c;
    Fm->kind = LSQ_MAT_DENSE;
    Fm->m = J->m;
    Fm->n = J->br_ng;
    Fm->nnz = (long long)J->m * J->br_ng;
    Fm->d_dense = s->d_work + l.F;
    s->inner_J = Fm;
    return LSQ_OK;
}

template <int G, int H>
static int bdq_factor(lsq_ctx *c, lsq_solver *s, lsq_mat *J, const double *d_y, const double *d_damp, const BdqLayout &l) {
    const int B = s->br_blocks;
    double *wk = s->d_work;
    const size_t lds = (G == 4 ? 1 : 4) * bdq_factor_doubles(s->br_nb, H) * sizeof(double);
    LSQ_TRY(lsq_set_lds(c, (const void *)k_bdq_factor<G, H>, lds));
    LSQ_LAUNCH((k_bdq_factor<G, H>), dim3(G == 4 ? B : (B + 3) / 4), dim3(256), lds, c->stream, B, s->br_mb, s->br_nb,
               (const double *)J->csc.d_val, J->d_colscale, d_y, d_damp, wk + l.R, wk + l.z, wk + l.r, wk + l.V, wk + l.T,
               s->d_info);
    const size_t lda = bdq_apply_doubles(s->br_nb, H) * sizeof(double);
    LSQ_TRY(lsq_set_lds(c, (const void *)k_bdq_apply<H>, lda));
    LSQ_LAUNCH((k_bdq_apply<H>), dim3(B, (s->br_ng + BDQ_TW - 1) / BDQ_TW), dim3(256), lda, c->stream, B, s->br_mb, s->br_nb,
               s->br_ng, (const double *)J->csc.d_val, J->d_colscale, (const double *)(wk + l.V), (const double *)(wk + l.T),
               (const int *)s->d_info, wk + l.W, wk + l.F);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

// the elimination of the locals, enqueued: k_bdq_init, k_bdq_factor, k_bdq_apply (also lsq_bordered_qr_covariance,
// lsq_cov_bordered.hip, with zeros for d_y and d_damp).  view (optional): where R, W and F stand in s->d_work
int lsq_borderedqr_eliminate(lsq_solver *s, lsq_mat *J, const double *d_y, const double *d_damp, LsqBdqView *view) {
    lsq_ctx *c = s->ctx;
    const int nb = s->br_nb;
    const BdqLayout l = bdq_layout(s->br_blocks, s->br_mb, nb, s->br_ng);
    LSQ_LAUNCH(k_bdq_init, dim3(1), dim3(64), 0, c->stream, s->d_info);
    if (nb > 16) LSQ_TRY(l.H == 64 ? (bdq_factor<4, 64>(c, s, J, d_y, d_damp, l)) : (bdq_factor<4, 32>(c, s, J, d_y, d_damp, l)));
    else LSQ_TRY(l.H == 64 ? (bdq_factor<1, 64>(c, s, J, d_y, d_damp, l)) : (bdq_factor<1, 32>(c, s, J, d_y, d_damp, l)));
    if (view) {
        view->R = s->d_work + l.R;
        view->W = s->d_work + l.W;
        view->F = s->d_work + l.F;
    }
    return LSQ_OK;
}

int lsq_borderedqr_solve(lsq_solver *s, lsq_mat *J, const double *d_y, const double *d_damp, double *d_x, int *nmul) {
    lsq_ctx *c = s->ctx;
    if (!d_damp) return lsq_bordered_refuse_dogleg();
    if (J->kind != LSQ_MAT_CSC || J->br_blocks != s->br_blocks || J->br_mb != s->br_mb || J->br_nb != s->br_nb ||
        J->br_ng != s->br_ng || J->m != s->m || J->n != s->n) {
        lsq_set_error("BorderedQR(): this solver was allocated for a bordered block-diagonal Jacobian of %d blocks of %d x %d "
                      "with %d shared columns; create a solver on the handle it is to solve with", s->br_blocks, s->br_mb,
                      s->br_nb, s->br_ng);
        return LSQ_EARG;
    }
    LSQ_HIP(hipSetDevice(c->device));
    LSQ_TRY(lsq_ensure_csc(J));        // (a device-side g! may have written the product mirrors only)
    const int B = s->br_blocks, mb = s->br_mb, nb = s->br_nb, ng = s->br_ng;
    const BdqLayout l = bdq_layout(B, mb, nb, ng);
    double *wk = s->d_work;
    double *xg = d_x + (size_t)B * nb;
    LSQ_TRY(lsq_borderedqr_eliminate(s, J, d_y, d_damp, nullptr));
    // min || [F; diag(sqrt(damp_g))] x_g - [r; 0] ||: the inner QR()'s damped solve, its rank decision and its retries
    LSQ_TRY(lsq_qr_solve(s->inner, s->inner_J, wk + l.r, d_damp + (size_t)B * nb, xg, nullptr));
    const size_t lds_back = ((size_t)nb * (nb | 1) + 256) * sizeof(double);
    LSQ_LAUNCH(k_bdq_back, dim3(B), dim3(256), lds_back, c->stream, B, nb, ng, (const double *)(wk + l.R),
               (const double *)(wk + l.z), (const double *)(wk + l.W), (const double *)xg, d_x);
    LSQ_HIP(hipGetLastError());
    s->last_bd_path = 6;
    s->last_bd_block = -1;
    if (nmul) *nmul = 1;
    int st4[4] = {0, 0, 0, 0};
    LSQ_TRY(lsq_read_ints(c, s->d_info, nullptr, nullptr, nullptr, st4));     // the one wait of the solve: the locals' verdict
    if (st4[0] != INT_MAX) {
        s->last_bd_block = (st4[0] - 1) / nb;
        lsq_set_error("RankDeficientException: BorderedQR(): the triangular factor of the local columns has a zero or non-finite "
                      "diagonal entry at column %d (a zero damping value on a zero column, or a non-finite operand)", st4[0]);
        return LSQ_ERANK;
    }
    return LSQ_OK;
}
