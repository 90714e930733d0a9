// BlockQR(): column-pivoted QR per block of a block-diagonal Jacobian J = blkdiag(J_1 .. J_B) (lsq_blockdiag_create, nb <= 64).
//
// Per block b this is the reference's QR() on that block alone (dense_qr.jl:30-88): x_b = ldiv!(qr!(J_b, ColumnNorm()), y_b)
// with xGELSY's rank decision at rcond = min(mb, nb) eps, and for LevenbergMarquardt the same on [J_b; diag(sqrt(damp_b))]
// with right-hand side (y_b, 0) and rcond = nb eps.  The Gram matrix is never formed, and a rank-deficient, an all-zero or a
// wide block gets its minimum-norm solution: nothing here is an error.  One solve is ONE pass over the values and one launch.
//
// Stage 1, streaming: the rows of J_b arrive in chunks of H rows (loaded down the columns, the next chunk's loads in flight)
// and every chunk is eliminated against the running upper-triangular R (nb x nb, LDS) by Householder reflectors that touch
// only R_jj and column j of the chunk (the triangle-over-rectangle step of TSQR); y_b is carried as column nb, so that column
// ends up holding c = Q'y.  LM's rows diag(sqrt(damp_b)) are the last chunk(s).  r_b = J_b'y_b and diag(J_b'J_b) -- what the
// batched trust-region loop wants from the same pass -- are summed from the staged chunks in a fixed order.
// Stage 2, in LDS: dgeqp3 (the dlaqp2 recurrence with its partial-norm downdate and tol3z recomputation) on R with c carried
// along -- in exact arithmetic the pivots of R are those of J_b --, the dlaic1 rank decision, the triangular solve, the RZ
// completion (dlatrz / dormr3) when rank < nb, and the un-permutation: k_qrcp_solve (lsq_qr.hip) restated for one block.
//
// Geometry as k_bd_solve: 16 < nb <= 64: one 256-thread workgroup per block (G = 4 wavefronts); nb <= 16: one wavefront per
// block, four blocks per workgroup (G = 1; the wavefronts of such a workgroup never meet at a barrier, so a block's arithmetic
// does not depend on its neighbours).  Threads work in groups of four ("quads"): a quad owns one column of the step at hand,
// its four threads own the rows r = q (mod 4) and combine their partial sums with two lane exchanges.  Every sum has a fixed
// order, there are no floating-point atomics and no hand-offs other than the barrier: two runs give identical bits, and
// block b's bits do not depend on B.
#include <cfloat>

#include "lsq_solver.h"
#include "lsq_laic1.h"
#include "lsq_bq.h"      // bq_sync, bq_quad_sum, bq_larfg

constexpr double BQ_MIN_DIAGONAL = 1e-6, BQ_MAX_DIAGONAL = 1e32;   // levenberg_marquardt.jl:85 (per-block damping, `delta`)

// doubles of LDS per block: R with the right-hand side as column nb (column stride nb | 1) | chunk (nb + 1 columns of H + 1)
// | vn1 vn2 (partial column norms) | dg (diag(J'J)) | sd (sqrt of the damping)
__host__ __device__ static inline size_t bq_group_doubles(int nb, int H) {
    return (size_t)(nb | 1) * (nb + 1) + (size_t)(nb + 1) * (H + 1) + 4 * (size_t)nb;
}

template <int G, int H>
__global__ void __launch_bounds__(256)
k_bq_solve(int B, int mb, int nb, const double *__restrict__ vals, const double *__restrict__ scale,
           const double *__restrict__ y, const double *__restrict__ damp, double *__restrict__ x, int *__restrict__ ranks,
           const int *__restrict__ active, double *__restrict__ r_out, double *__restrict__ diag_out,
           const double *__restrict__ delta) {
    // damp: nb damping values per block (lsq_ldiv_damped); delta: LM with one trust region per block, the damping of
    // levenberg_marquardt.jl:84-86 is formed here from the block's own diagonal; both null: the undamped solve.
    // active / r_out / diag_out: the batched loop's operands, as in k_bd_solve (an inactive block is left alone).
    extern __shared__ double bq_lds[];
    constexpr int GT = 64 * G, HQ = H / 4, CS = H + 1, CP = GT / H;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int gt = G == 4 ? tid : lane;                                  // thread inside its group
    const int b = G == 4 ? (int)blockIdx.x : (int)blockIdx.x * 4 + wv;
    if (b >= B || (active && active[b] == 0)) return;      // (G == 4: the same answer in every thread of the workgroup)
    const int ls = nb | 1;
    double *R = bq_lds + (G == 4 ? 0 : wv) * bq_group_doubles(nb, H);
    double *ch = R + ls * (nb + 1);
    double *vn1 = ch + (nb + 1) * CS, *vn2 = vn1 + nb, *dg = vn2 + nb, *sd = dg + nb;
    const bool damped = damp != nullptr || delta != nullptr;
    const bool byprod = r_out != nullptr || diag_out != nullptr || delta != nullptr;
    const int mtot = mb + (damped ? nb : 0);
    const int mn = mtot < nb ? mtot : nb;
    const int qi = gt >> 2, q = gt & 3;                    // quad, thread inside it
    const size_t vbase = (size_t)b * mb * nb, ybase = (size_t)b * mb, xbase = (size_t)b * nb;

    for (int e = gt; e < ls * (nb + 1); e += GT) R[e] = 0.0;

    // ---- one chunk (H rows x (nb + 1) columns, staged as [column][row]) against R: nb reflectors ----
    auto eliminate = [&]() {
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
            bq_sync<G>();
            if (gt == 0) R[j * ls + j] = beta;             // (read as alpha by every thread in front of the barrier)
        }
    };

    // ---- stage 1: stream J_b ----
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
    double dacc = 0.0, racc = 0.0;
    const int nch = (mb + H - 1) / H;
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
        if (byprod && qi < nb) {
#pragma unroll
            for (int t = 0; t < HQ; ++t) {
                const double a = ch[qi * CS + q + 4 * t];
                dacc += a * a;
                racc += a * ch[nb * CS + q + 4 * t];
            }
        }
        if (byprod) bq_sync<G>();      // step 0 of the elimination overwrites columns that other wavefronts read above
        eliminate();
    }
    if (byprod) {
        dacc = bq_quad_sum(dacc);
        racc = bq_quad_sum(racc);
        if (qi < nb && q == 0) {
            dg[qi] = dacc;
            if (diag_out) diag_out[xbase + qi] = dacc;
            if (r_out) r_out[xbase + qi] = racc;
        }
    }
    if (damped) {
        bq_sync<G>();
        if (delta) {                   // sum(dtd_b) in index order, every thread its own copy (LDS broadcast reads)
            double dsum = 0.0;
            for (int k = 0; k < nb; ++k) dsum += dg[k];
            if (gt < nb) {
                const double mean = dsum / nb, d = dg[gt];
                const double lo = BQ_MIN_DIAGONAL * mean, hi = BQ_MAX_DIAGONAL * mean;
                const double dc = d > hi ? hi : (d < lo ? lo : d);
                sd[gt] = sqrt(dc * (1.0 / delta[b]));
            }
        } else if (gt < nb) sd[gt] = sqrt(damp[xbase + gt]);
        bq_sync<G>();
        for (int c = 0; c * H < nb; ++c) {                 // the rows diag(sqrt(damp_b)), right-hand side 0
            const int vrow = c * H + lr;
#pragma unroll
            for (int p = 0; p < HQ; ++p) {
                const int col = c0 + p * CP;
                if (col < nb) ch[col * CS + lr] = col == vrow ? sd[col] : 0.0;
            }
            if (gt < H) ch[nb * CS + gt] = 0.0;
            bq_sync<G>();
            eliminate();
        }
    }
    bq_sync<G>();

    // ---- stage 2: dgeqp3 on R (nb rows, mn steps), c = column nb carried along ----
    const double tol3z = sqrt(DBL_EPSILON / 2);
    {
        double s = 0.0;
        if (qi < nb)
            for (int r = q; r < nb; r += 4) { const double a = R[qi * ls + r]; s += a * a; }
        s = bq_quad_sum(s);
        if (qi < nb && q == 0) { const double v = sqrt(s); vn1[qi] = v; vn2[qi] = v; }
    }
    int jp = lane;                     // the permutation, lane = position (every wavefront keeps its own copy)
    bq_sync<G>();
    for (int i = 0; i < mn; ++i) {
        double d = (lane >= i && lane < nb) ? vn1[lane] : -1.0;      // idamax: first maximum
        int idx = lane;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double od = __shfl_xor(d, off);
            const int oi = __shfl_xor(idx, off);
            if (od > d || (od == d && oi < idx)) { d = od; idx = oi; }
        }
        const int p = __builtin_amdgcn_readfirstlane(idx);
        bq_sync<G>();
        if (p != i) {
            if (gt < nb) { const double t = R[p * ls + gt]; R[p * ls + gt] = R[i * ls + gt]; R[i * ls + gt] = t; }
            if (gt == 0) { vn1[p] = vn1[i]; vn2[p] = vn2[i]; }
            const int ji = __builtin_amdgcn_readlane(jp, i), jq = __builtin_amdgcn_readlane(jp, p);
            if (lane == i) jp = jq;
            if (lane == p) jp = ji;
        }
        bq_sync<G>();
        double s2 = 0.0;               // dlarfg on R(i:nb-1, i), every quad its own copy
        for (int r = i + 1 + q; r < nb; r += 4) { const double a = R[i * ls + r]; s2 += a * a; }
        s2 = bq_quad_sum(s2);
        double tau, sc, beta;
        bq_larfg(R[i * ls + i], s2, &tau, &sc, &beta);
        const int k = i + 1 + qi;
        const bool on = k <= nb;
        double dot = 0.0;
        if (on && tau != 0.0)
            for (int r = i + 1 + q; r < nb; r += 4) dot += (R[i * ls + r] * sc) * R[k * ls + r];
        dot = bq_quad_sum(dot);
        double rik = on ? R[k * ls + i] : 0.0;
        if (on && tau != 0.0) {
            const double tw = tau * (dot + rik);
            for (int r = i + 1 + q; r < nb; r += 4) R[k * ls + r] -= (R[i * ls + r] * sc) * tw;
            rik -= tw;
            if (q == 0) R[k * ls + i] = rik;
        }
        bool rec = false;              // partial column norm downdate (dlaqp2)
        if (on && k < nb) {
            const double v1 = vn1[k];
            if (v1 != 0.0) {
                const double rr = fabs(rik) / v1;
                const double temp = fmax(1.0 - rr * rr, 0.0);
                const double qq = v1 / vn2[k];
                rec = temp * qq * qq <= tol3z;
                if (!rec && q == 0) vn1[k] = v1 * sqrt(temp);
            }
        }
        double a2 = 0.0;
        if (rec)
            for (int r = i + 1 + q; r < nb; r += 4) { const double a = R[k * ls + r]; a2 += a * a; }
        a2 = bq_quad_sum(a2);
        if (rec && q == 0) { const double nv = i < nb - 1 ? sqrt(a2) : 0.0; vn1[k] = nv; vn2[k] = nv; }
        bq_sync<G>();
        if (gt == 0) R[i * ls + i] = beta;
    }
    bq_sync<G>();

    // ---- rank decision (dlaic1), estimate vectors in registers (lane = entry), every wavefront its own copy ----
    const double rcond = mn * DBL_EPSILON;
    int rnk = 0;
    {
        double smax = fabs(R[0]), smin = smax;
        if (smax != 0.0) {
            double wmin = lane == 0 ? 1.0 : 0.0, wmax = wmin;
            rnk = 1;
            while (rnk < mn) {
                const double ck = lane < rnk ? R[rnk * ls + lane] : 0.0;
                const double a1 = wave_sum(wmin * ck), a2 = wave_sum(wmax * ck);
                const double gamma = R[rnk * ls + rnk];
                double sminpr, s1, c1, smaxpr, s2, c2;
                laic1_dev(2, a1, smin, gamma, &sminpr, &s1, &c1);
                laic1_dev(1, a2, smax, gamma, &smaxpr, &s2, &c2);
                if (smaxpr * rcond > sminpr) break;
                if (lane < rnk) { wmin *= s1; wmax *= s2; }
                if (lane == rnk) { wmin = c1; wmax = c2; }
                smin = sminpr; smax = smaxpr;
                rnk += 1;
            }
        }
    }
    // The solve is one wavefront's: lane = unknown, no barrier from here on.  Wavefront 0 may start rewriting R (dlatrz)
    // while the others are still in their own copy of the loop above: they only read, drop what they computed and return.
    if (G == 4 && wv != 0) return;
    const bool in = lane < nb;
    if (rnk == 0) {                    // all-zero block
        if (in) x[xbase + lane] = 0.0;
        if (lane == 0) ranks[b] = 0;
        return;
    }
    double z = in ? R[nb * ls + lane] : 0.0;               // c = Q'y
    double tzr = 0.0;
    if (rnk < nb) {
        // RZ factorisation of R(0:rnk, :) in place (dlatrz): [R11 R12] = [T 0] Z
        for (int i = rnk - 1; i >= 0; --i) {
            const bool tail = lane >= rnk && in;           // lane = column of R12
            double e = tail ? R[lane * ls + i] : 0.0;
            const double s2 = wave_sum(e * e);
            double tz, sc, beta;
            bq_larfg(R[i * ls + i], s2, &tz, &sc, &beta);
            if (lane == i) tzr = tz;
            if (tz != 0.0) {
                if (tail) R[lane * ls + i] = e * sc;
                if (lane == 0) R[i * ls + i] = beta;
            }
            bq_sync<1>();
            if (tz != 0.0 && lane < i) {                   // dlarz 'R' on rows 0 .. i-1, lane = row
                double w = R[i * ls + lane];
                for (int k = rnk; k < nb; ++k) w += R[k * ls + lane] * R[k * ls + i];
                R[i * ls + lane] -= tz * w;
                for (int k = rnk; k < nb; ++k) R[k * ls + lane] -= tz * w * R[k * ls + i];
            }
            bq_sync<1>();
        }
    }
    for (int k = rnk - 1; k >= 0; --k) {                   // T z = c(0:rnk) (rank nb: R z = c)
        const double u = lane < k ? R[k * ls + lane] : 0.0;
        const double xk = lsq_readlane_f64(z, k) / R[k * ls + k];
        if (lane == k) z = xk;
        else if (lane < k) z -= u * xk;
    }
    if (rnk < nb) {
        const bool tail = lane >= rnk && in;
        if (lane >= rnk) z = 0.0;
        for (int i = 0; i < rnk; ++i) {                    // Z'z (dormr3 'L','T')
            const double e = tail ? R[lane * ls + i] : 0.0;
            const double w = (lsq_readlane_f64(z, i) + wave_sum(e * z)) * lsq_readlane_f64(tzr, i);
            if (tail) z -= e * w;
            if (lane == i) z -= w;
        }
    }
    if (in) x[xbase + jp] = z;                             // un-permutation
    if (lane == 0) ranks[b] = rnk;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
int lsq_blockqr_solver_alloc(lsq_solver *s, const lsq_mat *J) {
    if (J->kind != LSQ_MAT_CSC || J->bd_blocks < 1) {
        lsq_set_error("BlockQR() needs a block-diagonal Jacobian (lsq_blockdiag_create) with blocks of at most 64 columns: "
                      "this %d x %d handle has no block shape. Use QR() on a dense Jacobian, LSMR() on a sparse one", J->m, J->n);
        return LSQ_EARG;
    }
    if (J->bd_nb > 64) {
        lsq_set_error("BlockQR() needs blocks of at most 64 columns (got %d blocks of %d x %d): one block's triangular factor "
                      "must fit the in-LDS factorisation. Use LSMR()", J->bd_blocks, J->bd_mb, J->bd_nb);
        return LSQ_EARG;
    }
    s->bd_blocks = J->bd_blocks;
    s->bd_mb = J->bd_mb;
    s->bd_nb = J->bd_nb;
    LSQ_HIP(hipMalloc(&s->d_info, (size_t)J->bd_blocks * sizeof(int)));      // the block ranks of the last solve
    return LSQ_OK;
}

// The chunk height is a launch-time choice: 64 rows when the block (with LM's rows) has more than 32, else 32.  At nb = 64
// that is 8706 doubles = 68 KB per workgroup, so two workgroups share a CU's 160 KB of LDS; four blocks of nb = 16: 46 KB.
template <int G, int H>
static int bq_launch(lsq_ctx *c, lsq_mat *J, const double *d_y, const double *d_damp, double *d_x, int *d_ranks,
                     const int *d_active, double *d_r, double *d_diag, const double *d_delta) {
    const int B = J->bd_blocks;
    const size_t lds = (G == 4 ? 1 : 4) * bq_group_doubles(J->bd_nb, H) * sizeof(double);
    LSQ_TRY(lsq_set_lds(c, (const void *)k_bq_solve<G, H>, lds));
    const int grid = G == 4 ? B : (B + 3) / 4;
    LSQ_LAUNCH((k_bq_solve<G, H>), dim3(grid), dim3(256), lds, c->stream, B, J->bd_mb, J->bd_nb, (const double *)J->csc.d_val,
               J->d_colscale, d_y, d_damp, d_x, d_ranks, d_active, d_r, d_diag, d_delta);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

static int bq_dispatch(lsq_ctx *c, lsq_mat *J, const double *d_y, const double *d_damp, double *d_x, int *d_ranks,
                       const int *d_active, double *d_r, double *d_diag, const double *d_delta) {
    const bool wide = J->bd_nb > 16;
    const int rows = (d_damp || d_delta) && J->bd_nb > J->bd_mb ? J->bd_nb : J->bd_mb;    // the longest run of rows
    const bool tall = rows > 32;
    if (wide) return tall ? bq_launch<4, 64>(c, J, d_y, d_damp, d_x, d_ranks, d_active, d_r, d_diag, d_delta)
                          : bq_launch<4, 32>(c, J, d_y, d_damp, d_x, d_ranks, d_active, d_r, d_diag, d_delta);
    return tall ? bq_launch<1, 64>(c, J, d_y, d_damp, d_x, d_ranks, d_active, d_r, d_diag, d_delta)
                : bq_launch<1, 32>(c, J, d_y, d_damp, d_x, d_ranks, d_active, d_r, d_diag, d_delta);
}

// One batched solve for the per-block trust-region loop (lsq_batched.hip), the twin of lsq_blockdiag_solve_blocks: lm: the
// damping is formed in the kernel from d_delta; else Dogleg's Gauss-Newton step.  d_ranks[b]: the rank of block b's solve.
int lsq_blockqr_solve_blocks(lsq_ctx *c, lsq_mat *J, bool lm, const double *d_y, const double *d_delta, double *d_x,
                             const int *d_active, int *d_ranks, double *d_r, double *d_diag) {
    LSQ_TRY(lsq_ensure_csc(J));
    return bq_dispatch(c, J, d_y, nullptr, d_x, d_ranks, d_active, d_r, d_diag, lm ? d_delta : nullptr);
}

// dense_qr.jl:30-42 (d_damp == nullptr) and :56-88 (damped) per block.  Nothing is read back: the ranks stay on the device
// until lsq_solver_info / lsq_solver_blockdiag_ranks ask for them.
int lsq_blockqr_solve(lsq_solver *s, lsq_mat *J, const double *d_y, const double *d_damp, double *d_x, int *nmul) {
    if (J->kind != LSQ_MAT_CSC || J->bd_blocks != s->bd_blocks || J->bd_mb != s->bd_mb || J->bd_nb != s->bd_nb ||
        J->m != s->m || J->n != s->n) {
        lsq_set_error("BlockQR: this solver was allocated for a block-diagonal Jacobian of %d blocks of %d x %d",
                      s->bd_blocks, s->bd_mb, s->bd_nb);
        return LSQ_EDIM;
    }
    LSQ_TRY(lsq_ensure_csc(J));        // (a device-side g! may have written the product mirrors only)
    LSQ_TRY(bq_dispatch(s->ctx, J, d_y, d_damp, d_x, s->d_info, nullptr, nullptr, nullptr, nullptr));
    s->last_bd_path = 3;
    s->last_bd_block = -1;
    s->bq_solved = true;
    if (nmul) *nmul = 1;
    return LSQ_OK;
}

extern "C" int lsq_solver_blockdiag_ranks(const lsq_solver *s, int *h_ranks) {
    if (!s || !h_ranks) { lsq_set_error("lsq_solver_blockdiag_ranks: null argument"); return LSQ_EARG; }
    if (s->kind != LSQ_BLOCK_QR) {
        lsq_set_error("lsq_solver_blockdiag_ranks: per-block ranks belong to BlockQR() (this solver's kind is %d)", s->kind);
        return LSQ_EARG;
    }
    if (!s->bq_solved) {
        for (int b = 0; b < s->bd_blocks; ++b) h_ranks[b] = -1;
        return LSQ_OK;
    }
    LSQ_HIP(hipStreamSynchronize(s->ctx->stream));
    LSQ_HIP(hipMemcpy(h_ranks, s->d_info, (size_t)s->bd_blocks * sizeof(int), hipMemcpyDeviceToHost));
    return LSQ_OK;
}
