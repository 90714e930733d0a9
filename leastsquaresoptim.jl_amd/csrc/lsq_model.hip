// The built-in device-side tanh model used by the synthetic benchmarks: its f! and g!, and the hooks (lsq_loop.h) by which the
// trust-region loops of lsq_optimize.hip fuse its passes into theirs.
#include <algorithm>

#include "lsq_loop.h"
#include "lsq_spmv.h"

// ---------------------------------------------------------------------------------------------
// built-in model: r(x) = A tanh(x) - b ; J = A diag(1 - tanh(x)^2)      
// ---------------------------------------------------------------------------------------------
struct lsq_model {
    lsq_ctx *ctx;
    lsq_mat *J;
    // fused: J is a COLUMN-SCALED handle on the sliced layouts (lsq_mat_set_colscale): J's own storage holds A once, g! writes
    // the n factors s = 1 - tanh(x)^2 and nothing else; every product applies them on the fly
    bool fused = false;
    double *d_Acsc = nullptr;  // A values, CSC order (or dense column-major)                       } not fused: J's values are
    double *d_Acsr = nullptr;  // A values in J's row-mirror layout (CSR order or sliced rows)      } multiplied out by g!
    double *d_Ab = nullptr;    // A values in J's column-mirror layout (window-blocked CSC or sliced columns)
    double *d_b = nullptr;
    double *d_t = nullptr;     // tanh(x) of the latest f!
    double *d_s = nullptr;     // 1 - tanh(x)^2 of the latest g! (fused: this IS J's column scale)
    double *d_sspec = nullptr; // the same at the latest trial point (written by the step kernel)
    const double *tanh_x = nullptr;   // device vector whose tanh the step kernel has already put into d_t
    const double *sfac_x = nullptr;   // device vector whose 1 - tanh^2 the step kernel has already put into d_sspec
    // k_sell_rows_pair reads its two m-vectors in the SLICE ORDER of J's sliced rows (lsq_sell.h): b once, and two mirrors of
    // residual vectors, each valid for the row-order device vector named in perm_of (nullptr: stale)
    double *d_b_perm = nullptr;
    double *d_perm[2] = {nullptr, nullptr};
    const double *perm_of[2] = {nullptr, nullptr};
    long long pair_tails = 0;  // launches of k_sell_rows_pair (lsq_model_paths)
};
static void model_perm_invalidate(lsq_model *md, const double *vec) {   // vec == nullptr: all
    for (int k = 0; k < 2; ++k)
        if (!vec || md->perm_of[k] == vec) md->perm_of[k] = nullptr;
}

__global__ void __launch_bounds__(LSQ_NT) k_tanh(int n, const double *__restrict__ x, double *__restrict__ t) {
    for (int i = blockIdx.x * LSQ_NT + threadIdx.x; i < n; i += gridDim.x * LSQ_NT) t[i] = tanh(x[i]);
}

struct EpiResidual {  // out = A t - b
    static constexpr bool REDUCE = false;
    const int *done;
    int extra_blocks;
    const double *b;
    double *out;
    double *partials;
    unsigned *counter;
    __device__ void seg(int i, double dot, double &) const { out[i] = dot - b[i]; }
    using has_pre = void;
    __device__ double pre(int i) const { return b[i]; }
    __device__ void seg_pre(int i, double dot, double bi, double &) const { out[i] = dot - bi; }
    __device__ void extra(int, double &) const {}
    __device__ void finalize(double) const {}
};

struct EpiResidualSq {  // out = A t - b, and sum(out.^2) -> slot (+ the iteration's scalars to the host, like EpiPredict)
    static constexpr bool REDUCE = true;
    const int *done;
    int extra_blocks;
    const double *b;
    double *out;
    double *partials;
    unsigned *counter;
    double *slot;
    LsqSlotPublish pub;
    __device__ void seg(int i, double dot, double &racc) const { seg_pre(i, dot, b[i], racc); }
    using has_pre = void;
    __device__ double pre(int i) const { return b[i]; }
    __device__ void seg_pre(int i, double dot, double bi, double &racc) const {
        const double v = dot - bi;
        out[i] = v;
        racc += v * v;
    }
    __device__ void extra(int, double &) const {}
    __device__ void finalize(double t) const {
        *slot = t;
        if (pub.count > 0) {
            for (int i = 0; i < pub.count; ++i)
                __hip_atomic_store(pub.dst + i, pub.src + i == slot ? t : pub.src[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(pub.seq_word, pub.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
};

// ... and the same residual in the SLICE ORDER of the sliced rows (what k_sell_rows_pair reads: SellPairEpi), stored by the lane
// that formed the row's sum: out_perm[s * 64 + lane] = dot - b_perm[s * 64 + lane], the bits of out[row]
struct EpiResidualSqPerm : EpiResidualSq {
    const double *b_perm;
    double *out_perm;
    using has_slice_out = void;
    __device__ double slice_pre(size_t pidx) const { return b_perm[pidx]; }
    __device__ void slice_post(size_t pidx, double dot, double bi) const { out_perm[pidx] = dot - bi; }
};

// column scaling of a column-segmented value array (CSC nzval or dense columns)
__global__ void __launch_bounds__(LSQ_NT)
k_scale_cols(int n, const int *__restrict__ colptr, int m_dense, const double *__restrict__ A,
             const double *__restrict__ x, double *__restrict__ out) {
    for (int j = blockIdx.x; j < n; j += gridDim.x) {
        double t = tanh(x[j]);
        double s = 1.0 - t * t;
        long long k0 = colptr ? colptr[j] : (long long)j * m_dense;
        long long k1 = colptr ? colptr[j + 1] : (long long)(j + 1) * m_dense;
        for (long long k = k0 + threadIdx.x; k < k1; k += LSQ_NT) out[k] = A[k] * s;
    }
}
// dense J = A diag(1 - tanh(x)^2): block (column j, row chunk)
__global__ void __launch_bounds__(LSQ_NT)
k_scale_dense(int m, const double *__restrict__ A, const double *__restrict__ x, double *__restrict__ out) {
    const int j = blockIdx.x;
    const double t = tanh(x[j]);
    const double sfac = 1.0 - t * t;
    const size_t base = (size_t)j * m;
    for (int i = blockIdx.y * LSQ_NT + threadIdx.x; i < m; i += gridDim.y * LSQ_NT) out[base + i] = A[base + i] * sfac;
}
// the CSR mirror: scale by the column of each entry
__global__ void __launch_bounds__(LSQ_NT)
k_scale_csr(long long nnz, const int *__restrict__ colidx, const double *__restrict__ A, const double *__restrict__ sfac,
            double *__restrict__ out) {
    for (long long k = blockIdx.x * (long long)LSQ_NT + threadIdx.x; k < nnz; k += (long long)gridDim.x * LSQ_NT)
        out[k] = A[k] * sfac[colidx[k]];
}
// the start point of a solve: t = tanh(x), s = 1 - tanh(x)^2 (k_tanh and k_sfac, the same expressions) and check_isfinite(x)
// (k_first_nonfinite, the same code) in one launch
__global__ void __launch_bounds__(LSQ_NT) k_tanh_sfac(int n, const double *__restrict__ x, double *__restrict__ t,
                                                      double *__restrict__ s, double *partials, unsigned *counter,
                                                      double *out_nonfin) {
    __shared__ double sh[LSQ_NT / 64];
    double code = 0.0;
    for (int i = blockIdx.x * LSQ_NT + threadIdx.x; i < n; i += gridDim.x * LSQ_NT) {
        const double xi = x[i];
        const double v = tanh(xi);
        t[i] = v;
        s[i] = 1.0 - v * v;
        if (!isfinite(xi) && code == 0.0) code = 1e15 - (double)(i + 1);
    }
    const double bv = block_max<LSQ_NT>(code, sh);
    grid_reduce<LSQ_NT, true>(bv, partials, counter, gridDim.x, sh, [=](double m) {
        *out_nonfin = (m == 0.0) ? -1.0 : (1e15 - m) - 1.0;
    });
}
__global__ void __launch_bounds__(LSQ_NT) k_sfac(int n, const double *__restrict__ x, double *__restrict__ s) {
    for (int i = blockIdx.x * LSQ_NT + threadIdx.x; i < n; i += gridDim.x * LSQ_NT) {
        double t = tanh(x[i]);
        s[i] = 1.0 - t * t;
    }
}

// window-blocked CSC: segment s belongs to column s % n; one wave per segment
__global__ void __launch_bounds__(LSQ_NT)
k_scale_bcsc(int nseg, int n, const int *__restrict__ ptr, const double *__restrict__ A, const double *__restrict__ sfac,
             double *__restrict__ out) {
    const int lane = threadIdx.x & 63, per = LSQ_NT / 64;
    for (int s = blockIdx.x * per + (threadIdx.x >> 6); s < nseg; s += gridDim.x * per) {
        const double f = sfac[s % n];
        const int k1 = ptr[s + 1];
        for (int k = ptr[s] + lane; k < k1; k += 64) out[k] = A[k] * f;
    }
}

// out[k] = A[k] * sfac[col16[k]] with the n scale factors staged in LDS: pure streaming
// (16-byte value loads/stores, 8-byte index loads), one persistent 1024-thread workgroup per CU.
// NT: the output is stored non-temporally (16-byte vector stores: 4.8 TB/s instead of 3.8 -- no
// write-allocate next to the A stream); used for the copy that is not read back right away.
typedef double lsq_d2 __attribute__((ext_vector_type(2)));
template <bool NT>
__global__ void __launch_bounds__(1024)
k_scale_lds(long long nnz4, const unsigned short *__restrict__ col16, const double *__restrict__ A,
            const double *__restrict__ sfac, int n, double *__restrict__ out) {
    extern __shared__ double sf[];
    // (the factors 1 - tanh(x)^2 come from k_sfac: ten fp64 tanh per thread in every one of the 256
    //  workgroups cost ~6 us before the first byte was streamed)
    for (int i = threadIdx.x; i < n; i += 1024) sf[i] = sfac[i];
    __syncthreads();
    for (long long q = blockIdx.x * 1024LL + threadIdx.x; q < nnz4; q += (long long)gridDim.x * 1024) {
        const long long k = 4 * q;  // arrays are padded to a multiple of 4 (+8)
        const lsq_d2 a0 = *reinterpret_cast<const lsq_d2 *>(A + k);
        const lsq_d2 a1 = *reinterpret_cast<const lsq_d2 *>(A + k + 2);
        const uint2 c = *reinterpret_cast<const uint2 *>(col16 + k);
        lsq_d2 o0, o1;
        o0.x = a0.x * sf[c.x & 0xffffu];
        o0.y = a0.y * sf[c.x >> 16];
        o1.x = a1.x * sf[c.y & 0xffffu];
        o1.y = a1.y * sf[c.y >> 16];
        if constexpr (NT) {
            __builtin_nontemporal_store(o0, reinterpret_cast<lsq_d2 *>(out + k));
            __builtin_nontemporal_store(o1, reinterpret_cast<lsq_d2 *>(out + k + 2));
        } else {
            *reinterpret_cast<lsq_d2 *>(out + k) = o0;
            *reinterpret_cast<lsq_d2 *>(out + k + 2) = o1;
        }
    }
}

// short segments (LDS-window plan: ~4 entries): one thread per segment
__global__ void __launch_bounds__(LSQ_NT)
k_scale_bcsc_thread(int nseg, int n, const int *__restrict__ ptr, const double *__restrict__ A,
                    const double *__restrict__ sfac, double *__restrict__ out) {
    for (int s = blockIdx.x * LSQ_NT + threadIdx.x; s < nseg; s += gridDim.x * LSQ_NT) {
        const double f = sfac[s % n];
        const int k1 = ptr[s + 1];
        for (int k = ptr[s]; k < k1; ++k) out[k] = A[k] * f;
    }
}

static int model_f(double *out, const double *x, void *user) {
    lsq_model *md = (lsq_model *)user;
    lsq_ctx *c = md->ctx;
    lsq_mat *J = md->J;
    const bool have_tanh = md->tanh_x == x;   // the step kernel formed tanh(x) while it wrote x (model_trial_buffers)
    md->tanh_x = nullptr;
    model_perm_invalidate(md, out);           // (a slice-order mirror of `out` is stale from here on)
    if (!have_tanh) {
        md->sfac_x = nullptr;
        LSQ_LAUNCH(k_tanh, dim3(ngrid(c, J->n)), dim3(LSQ_NT), 0, c->stream, J->n, x, md->d_t);
    }
    EpiResidual e{nullptr, 0, md->d_b, out, nullptr, nullptr};
    if (J->kind == LSQ_MAT_CSC && J->srows.active) {
        // the stored values themselves (fused: J's storage IS A; else A in the same layout), no column scale: r = A t - b
        if (launch_sell_rows(J, nullptr, md->d_t, e, md->fused ? nullptr : md->d_Acsr) != LSQ_OK) return 1;
    } else if (J->kind == LSQ_MAT_CSC) {
        LsqSegs A = J->csr;  // same pattern, A's values
        A.d_val = md->d_Acsr;
        if (launch_segs<false>(c, A, md->d_t, e) != LSQ_OK) return 1;
    } else {
        lsq_mat tmp = *J;
        tmp.d_dense = md->d_Acsc;
        if (launch_product(&tmp, 0, md->d_t, e) != LSQ_OK) return 1;
    }
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

// the step kernel of both loops writes tanh(x_trial) and 1 - tanh(x_trial)^2 next to x_trial itself: the model's f!(., x_trial)
// and -- if the step is accepted -- its g!(., x_trial) then need no n-length launch of their own
void model_trial_buffers(void *user, const double *xt, double **t_out, double **s_out) {
    lsq_model *md = (lsq_model *)user;
    md->tanh_x = md->sfac_x = nullptr;
    if ((md->J->kind == LSQ_MAT_CSC && md->J->srows.active) || md->J->kind == LSQ_MAT_DENSE) {
        *t_out = md->d_t;
        *s_out = md->d_sspec;
        md->tanh_x = md->sfac_x = xt;
    }
}

int model_start_point(void *user, const double *x, double *d_nonfin, bool *done) {
    lsq_model *md = (lsq_model *)user;
    lsq_ctx *c = md->ctx;
    lsq_mat *J = md->J;
    *done = false;
    md->tanh_x = md->sfac_x = nullptr;
    if (!(J->kind == LSQ_MAT_CSC && J->srows.active) || J->n <= 0) return 0;
    LSQ_LAUNCH(k_tanh_sfac, dim3(ngrid(c, J->n)), dim3(LSQ_NT), 0, c->stream, J->n, x, md->d_t, md->d_sspec, c->d_partials,
               lsq_ctr(c, 0), d_nonfin);
    if (hipGetLastError() != hipSuccess) return 1;
    md->tanh_x = md->sfac_x = x;      // (as model_trial_buffers records them for the step kernel)
    *done = true;
    return 0;
}
void model_forget_point(void *user) {
    lsq_model *md = (lsq_model *)user;
    md->tanh_x = md->sfac_x = nullptr;
}

// does model_pair_tail apply to this handle (its conditions on the model and the layout; the caller adds those on the vectors)
static bool model_pair_applies(const lsq_model *md, const lsq_mat *J) {
    return md->fused && J == md->J && J->kind == LSQ_MAT_CSC && J->srows.active && J->srows.ncw == 1 && J->d_colscale &&
           J->n <= LSQ_PAIR_X_MAX && !getenv("LSQ_NO_PAIR_TAIL");
}
// the slice-order buffers of model_pair_tail: b once per model, two mirrors of residual vectors.  false: they could not be
// allocated (the callers take the paths that do without)
static bool model_perm_ready(lsq_model *md) {
    if (md->d_b_perm) return true;
    lsq_ctx *c = md->ctx;
    const LsqSell &S = md->J->srows;
    const size_t plen = (size_t)S.nslices * 64;
    const int pgrid = std::max(1, std::min(lsq_div_up((long long)plen, LSQ_NT), c->num_cus * 8));
    double *pb = nullptr, *p0 = nullptr, *p1 = nullptr;     // (all three or none: a partial set must not look initialised)
    if (hipMalloc(&pb, plen * sizeof(double)) != hipSuccess || hipMalloc(&p0, plen * sizeof(double)) != hipSuccess ||
        hipMalloc(&p1, plen * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        hipFree(pb); hipFree(p0); hipFree(p1);
        return false;
    }
    md->d_b_perm = pb; md->d_perm[0] = p0; md->d_perm[1] = p1;
    LSQ_LAUNCH(k_sell_perm_rows<0>, dim3(pgrid), dim3(LSQ_NT), 0, c->stream, sell_dev(S), S.wrows, S.nslices, (const double *)md->d_b,
               md->d_b_perm);
    return true;
}

// f! + sum(abs2, out) in one pass (sliced rows only; *done tells whether it applied)
int model_f_sumsq(void *user, double *out, const double *x, int ctr, double *d_out, LsqSlotPublish pub, bool *done,
                         const int *skip, bool mirror) {
    lsq_model *md = (lsq_model *)user;
    lsq_ctx *c = md->ctx;
    lsq_mat *J = md->J;
    *done = false;
    if (!(J->kind == LSQ_MAT_CSC && J->srows.active)) return model_f(out, x, user);
    model_perm_invalidate(md, out);
    EpiResidualSq e{skip, 0, md->d_b, out, c->d_partials, lsq_ctr(c, ctr), d_out, pub};
    const bool have_tanh = md->tanh_x == x;   // k_step (or k_tanh_sfac at the start point) formed tanh(x)
    md->tanh_x = nullptr;
    if (!have_tanh) {
        md->sfac_x = nullptr;
        LSQ_LAUNCH(k_tanh, dim3(ngrid(c, J->n)), dim3(LSQ_NT), 0, c->stream, J->n, x, md->d_t);
    }
    if (mirror && !skip && model_pair_applies(md, J) && model_perm_ready(md)) {
        EpiResidualSqPerm ep;
        static_cast<EpiResidualSq &>(ep) = e;
        ep.b_perm = md->d_b_perm;
        ep.out_perm = md->d_perm[0];
        if (launch_sell_rows(J, nullptr, md->d_t, ep, nullptr) != LSQ_OK) return 1;
        md->perm_of[0] = out;       // (model_pair_tail finds it there; perm_of[1] names another vector or nothing: `out` was invalidated)
    } else if (launch_sell_rows(J, nullptr, md->d_t, e, md->fused ? nullptr : md->d_Acsr) != LSQ_OK) return 1;
    *done = true;
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int model_pair_tail(void *user, lsq_mat *J, const double *dx, const double *fcur, double *ftrial, const double *xt,
                           double *slot_pred, double *slot_trial, LsqSlotPublish pub, const int *skip, bool *done, SpecGrad *sg) {
    lsq_model *md = (lsq_model *)user;
    lsq_ctx *c = md->ctx;
    *done = false;
    // the column-scaled handle on the one-window sliced rows (J = A diag(s): both products stream the same A), both gather
    // vectors resident in LDS, tanh(x_trial) already formed by the step kernel
    if (!(model_pair_applies(md, J) && md->tanh_x == xt)) return 0;
    const LsqSell &S = J->srows;
    const int nxpad = (J->n + 1) & ~1;
    // (two gather vectors; after a block's stream their LDS is the output window of its LSQ_SELL_ROWS_MAX rows)
    const size_t lds = (size_t)std::max(2 * nxpad, LSQ_SELL_ROWS_MAX) * sizeof(double);
    if (lsq_set_lds(c, (const void *)k_sell_rows_pair<0>, (size_t)2 * LSQ_PAIR_X_MAX * sizeof(double)) != LSQ_OK) return 0;
    // slice-order mirrors: b once; f from the slot that mirrors fcur (filled by an earlier launch of this kernel if the step that
    // produced fcur was accepted, else permuted now); the other slot takes this launch's trial residual
    const size_t plen = (size_t)S.nslices * 64;
    const int pgrid = std::max(1, std::min(lsq_div_up((long long)plen, LSQ_NT), c->num_cus * 8));
    if (!model_perm_ready(md)) return 0;                        // (the caller takes the two-pass tail)
    int k = md->perm_of[0] == fcur ? 0 : (md->perm_of[1] == fcur ? 1 : -1);
    if (k < 0) {
        k = 0;
        LSQ_LAUNCH(k_sell_perm_rows<0>, dim3(pgrid), dim3(LSQ_NT), 0, c->stream, sell_dev(S), S.wrows, S.nslices, fcur, md->d_perm[k]);
        md->perm_of[k] = fcur;
    }
    md->perm_of[1 - k] = ftrial;
    md->tanh_x = nullptr;     // (consumed, as model_f_sumsq does)
    const int grid = std::max(1, std::min(S.nblocks, c->num_cus));
    // (the step kernel has put 1 - tanh^2(x_trial) into d_sspec: the factors g! will install if the step is accepted)
    const bool spec = sg && sg->gate && md->sfac_x == xt;
    SellPairEpi e{skip, md->d_perm[k], md->d_b_perm, ftrial, md->d_perm[1 - k], c->d_partials, c->d_partials + 4096, lsq_ctr(c, 7),
                  slot_pred, slot_trial, pub, spec ? sg->gate : nullptr, spec ? sg->ssr : 0.0, MIN_STEP_QUALITY,
                  c->d_slots + SL_SSR, c->d_slots + SL_DX, c->d_slots + SL_GRAD, spec ? sg->xtol : 0.0, spec ? sg->ftol : 0.0,
                  spec ? sg->gtol : 0.0};
    LSQ_LAUNCH(k_sell_rows_pair<0>, dim3(grid), dim3(LSQ_BIG_NT), lds, c->stream, sell_dev(S), S.wrows, J->m, dx, J->d_colscale,
               (const double *)md->d_t, J->n, nxpad, e);
    *done = true;
    ++md->pair_tails;
    if (hipGetLastError() != hipSuccess) return 1;
    if (spec) {
        const int st = lsq_sparse_grad_colsum_spec(J, ftrial, sg->grad, md->d_sspec, sg->gate);
        if (st == LSQ_OK) sg->launched = true;
        else if (st != LSQ_EARG) return 1;
    }
    return 0;
}

static int model_g(lsq_mat *J, const double *x, void *user) {
    lsq_model *md = (lsq_model *)user;
    lsq_ctx *c = md->ctx;
    // s = 1 - tanh(x)^2: already there if x is the trial point the step kernel has just written (dense columns: k_scale_dense
    // forms the factor of its column from x itself)
    if (J->kind == LSQ_MAT_DENSE) {}
    else if (md->sfac_x == x) std::swap(md->d_s, md->d_sspec);
    else LSQ_LAUNCH(k_sfac, dim3(ngrid(c, J->n)), dim3(LSQ_NT), 0, c->stream, J->n, x, md->d_s);
    md->sfac_x = nullptr;
    md->tanh_x = nullptr;
    if (md->fused) {
        // J = A diag(s) is never multiplied out: handing the handle its (new) factor vector is all of g!
        if (lsq_mat_set_colscale(J, md->d_s) != LSQ_OK) return 1;
        return hipGetLastError() == hipSuccess ? 0 : 1;
    }
    if (J->kind == LSQ_MAT_CSC) {
        // mirrors the products read: rows (CSR or sliced rows) and columns (window-blocked CSC or sliced
        // columns), each with a 16-bit column per stored entry when the LDS-staged scaling applies
        const bool have_cols = J->scols.active || J->nwin > 1;
        const unsigned short *rcol = J->srows.active ? J->srows.d_idx16 : J->csr.d_idx16;
        const unsigned short *ccol = J->scols.active ? J->scols.d_col16 : J->bcsc.d_col16;
        double *rval = J->srows.active ? J->srows.d_val : J->csr.d_val;
        double *cval = J->scols.active ? J->scols.d_val : J->bcsc.d_val;
        const long long rlen = lsq_mirror_rows_len(J), clen = lsq_mirror_cols_len(J);
        const bool lds_ok = J->n <= 12000 && J->nnz >= (1 << 20) && J->srows.ncw == 1;   // (window-relative indices otherwise)
        // big problems: every product (and colsumabs2) reads the mirrors, so only those are written; the
        // CSC-ordered copy is rebuilt on demand (lsq_ensure_csc)
        const bool lazy_csc = lds_ok && rcol && have_cols && ccol && lsq_can_fuse_grad_colsum(J);
        if (!lazy_csc) {
            int grid = J->n < c->num_cus * 16 ? (J->n > 0 ? J->n : 1) : c->num_cus * 16;
            LSQ_LAUNCH(k_scale_cols, dim3(grid), dim3(LSQ_NT), 0, c->stream, J->n, J->csc.d_ptr, 0, md->d_Acsc,
                               x, J->csc.d_val);
        }
        J->csc_fresh = !lazy_csc;
        const size_t lds = (size_t)J->n * sizeof(double);
        if (lds_ok) {
            LSQ_TRY(lsq_set_lds(c, (const void *)k_scale_lds<true>, 12000 * 8));
            LSQ_TRY(lsq_set_lds(c, (const void *)k_scale_lds<false>, 12000 * 8));
        }
        if (J->nnz > 0) {
            if (lds_ok && rcol) {
                LSQ_LAUNCH(k_scale_lds<true>, dim3(c->num_cus), dim3(1024), lds, c->stream, (rlen + 3) / 4, rcol,
                                   md->d_Acsr, md->d_s, J->n, rval);
            } else if (!J->srows.active) {
                long long g2 = std::min<long long>((J->nnz + LSQ_NT - 1) / LSQ_NT, (long long)c->num_cus * 16);
                LSQ_LAUNCH(k_scale_csr, dim3((int)g2), dim3(LSQ_NT), 0, c->stream, J->nnz, J->csr.d_idx,
                                   md->d_Acsr, md->d_s, J->csr.d_val);
            } else {
                // sliced rows without the LDS-staged scaling (forced onto a small pattern): rebuild from the CSC copy
                if (lazy_csc) return 1;
                if (lsq_mirror_rows(J, J->csc.d_val, rval) != LSQ_OK) return 1;
            }
        }
        if (have_cols) {
            if (lds_ok && ccol) {
                LSQ_LAUNCH(k_scale_lds<false>, dim3(c->num_cus), dim3(1024), lds, c->stream, (clen + 3) / 4,
                                   ccol, md->d_Ab, md->d_s, J->n, cval);
            } else if (J->scols.active) {
                // no LDS-staged scaling: rebuild the sliced columns from the CSC copy instead
                if (lazy_csc) return 1;
                if (lsq_mirror_cols(J, J->csc.d_val, cval) != LSQ_OK) return 1;
            } else if (J->nnz < 16LL * J->bcsc.nseg) {
                int nsegs = J->bcsc.nseg;
                int g3 = std::min(lsq_div_up(nsegs, LSQ_NT), c->num_cus * 16);
                LSQ_LAUNCH(k_scale_bcsc_thread, dim3(g3), dim3(LSQ_NT), 0, c->stream, nsegs, J->n,
                                   J->bcsc.d_ptr, md->d_Ab, md->d_s, J->bcsc.d_val);
            } else {
                int nsegs = J->bcsc.nseg;
                int g3 = std::min(lsq_div_up(nsegs, LSQ_NT / 64), c->num_cus * 16);
                LSQ_LAUNCH(k_scale_bcsc, dim3(g3), dim3(LSQ_NT), 0, c->stream, nsegs, J->n, J->bcsc.d_ptr,
                                   md->d_Ab, md->d_s, J->bcsc.d_val);
            }
        }
        J->csr_fresh = true;  // every mirror written directly: no permutation pass needed
    } else {
        // dense columns: every block takes a (column, row chunk) pair, so that a matrix with few columns still fills the chip
        const long long tot = (long long)J->m * J->n;
        const int chunks = std::max(1, (int)std::min<long long>((J->m + 4 * LSQ_NT - 1) / (4 * LSQ_NT),
                                                               std::max<long long>(1, (long long)c->num_cus * 16 / std::max(1, J->n))));
        if (tot > 0)
            LSQ_LAUNCH(k_scale_dense, dim3(J->n, chunks), dim3(LSQ_NT), 0, c->stream, J->m, md->d_Acsc, x, J->d_dense);
    }
    J->version++;
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

bool model_is_builtin(lsq_f_callback f, lsq_g_callback g) { return f == model_f && (!g || g == model_g); }

extern "C" lsq_f_callback lsq_model_f(void) { return model_f; }
extern "C" lsq_g_callback lsq_model_g(void) { return model_g; }

extern "C" int lsq_model_tanh_create(lsq_ctx *c, lsq_mat *J, const double *hA, const double *hb, lsq_model **out) {
    if (!c || !J || !hA || !hb || !out) return LSQ_EARG;
    LSQ_HIP(hipSetDevice(c->device));
    lsq_model *md = new lsq_model();
    md->ctx = c;
    md->J = J;
    const size_t nb = (size_t)(J->n > 0 ? J->n : 1) * sizeof(double);
    LSQ_HIP(hipMalloc(&md->d_b, (size_t)(J->m > 0 ? J->m : 1) * sizeof(double)));
    LSQ_HIP(hipMemcpy(md->d_b, hb, (size_t)J->m * sizeof(double), hipMemcpyHostToDevice));
    LSQ_HIP(hipMalloc(&md->d_t, nb));
    LSQ_HIP(hipMalloc(&md->d_s, nb));
    LSQ_HIP(hipMalloc(&md->d_sspec, nb));
    if (lsq_colscale_fusable(J)) {
        // J's own storage takes A (once, in every layout); from here on J = A diag(s) through the handle's column scale
        LSQ_TRY(lsq_mat_set_values(J, hA));
        LSQ_TRY(lsq_fill(c, J->n, 1.0, md->d_s));
        LSQ_TRY(lsq_mat_set_colscale(J, md->d_s));
        md->fused = true;
        LSQ_HIP(hipStreamSynchronize(c->stream));
        *out = md;
        return LSQ_OK;
    }
    size_t vb = (size_t)(J->nnz + 8) * sizeof(double);
    LSQ_HIP(hipMalloc(&md->d_Acsc, vb));
    LSQ_ZERO(md->d_Acsc, 0, vb);
    LSQ_HIP(hipMemcpy(md->d_Acsc, hA, (size_t)J->nnz * sizeof(double), hipMemcpyHostToDevice));
    if (J->kind == LSQ_MAT_CSC) {
        // A in the layouts the products of J read (same maps as J's own mirrors), permuted once
        const size_t rb = (size_t)(lsq_mirror_rows_len(J) + 1024) * sizeof(double);
        LSQ_HIP(hipMalloc(&md->d_Acsr, rb));
        LSQ_ZERO(md->d_Acsr, 0, rb);
        LSQ_TRY(lsq_mirror_rows(J, md->d_Acsc, md->d_Acsr));
        if (lsq_mirror_cols_len(J) > 0) {
            const size_t cbytes = (size_t)(lsq_mirror_cols_len(J) + 1024) * sizeof(double);
            LSQ_HIP(hipMalloc(&md->d_Ab, cbytes));
            LSQ_ZERO(md->d_Ab, 0, cbytes);
            LSQ_TRY(lsq_mirror_cols(J, md->d_Acsc, md->d_Ab));
        }
        LSQ_HIP(hipStreamSynchronize(c->stream));
    }
    *out = md;
    return LSQ_OK;
}

extern "C" int lsq_model_paths(const lsq_model *md, int *sliced_rows, int *sliced_cols, int *lsmr_path, long long *pair_tails) {
    if (!md || !sliced_rows || !sliced_cols || !lsmr_path || !pair_tails) {
        lsq_set_error("lsq_model_paths: null argument");
        return LSQ_EARG;
    }
    const lsq_mat *J = md->J;
    *sliced_rows = J->kind == LSQ_MAT_CSC && J->srows.active;
    *sliced_cols = J->kind == LSQ_MAT_CSC && J->scols.active;
    *lsmr_path = lsq_workspace_lsmr_path(md->ctx, J);
    *pair_tails = md->pair_tails;
    return LSQ_OK;
}

extern "C" int lsq_model_destroy(lsq_model *md) {
    if (!md) return LSQ_OK;
    hipStreamSynchronize(md->ctx->stream);
    if (md->fused && md->J) lsq_mat_set_colscale(md->J, nullptr);   // (the factor vector goes away with the model)
    hipFree(md->d_Acsc); hipFree(md->d_Acsr); hipFree(md->d_Ab); hipFree(md->d_b); hipFree(md->d_t); hipFree(md->d_s); hipFree(md->d_sspec);
    hipFree(md->d_b_perm); hipFree(md->d_perm[0]); hipFree(md->d_perm[1]);
    delete md;
    return LSQ_OK;
}
