// Solver plug point (ldiv!): the handle every solver kind sits behind, its public entries and path queries.  Host code only:
// the solves themselves live with their kernels (lsq_lsmr.hip, lsq_dense.hip, lsq_qr.hip, lsq_blockdiag.hip, ...).
#include "lsq_solver.h"

// ---------------------------------------------------------------------------------------------
// solver objects
// ---------------------------------------------------------------------------------------------
extern "C" int lsq_solver_create(lsq_ctx *c, lsq_mat *J, int kind, int for_lm, lsq_solver **out) {
    LSQ_RANGE("lsq_solver_create");
    if (!c || !J || !out) return LSQ_EARG;
    if (kind == LSQ_QR && J->kind != LSQ_MAT_DENSE) {
        lsq_set_error("solver QR() is not available for sparse Jacobians. Choose between Cholesky() and LSMR()");
        return LSQ_EARG;  // types.jl:115-117
    }
    const bool blockdiag = kind == LSQ_CHOLESKY && J->kind == LSQ_MAT_CSC && J->bd_blocks > 0;   // lsq_blockdiag_create
    const bool bordered = kind == LSQ_CHOLESKY && J->kind == LSQ_MAT_CSC && J->br_blocks > 0;   // lsq_blockdiag_bordered_create
    if (kind == LSQ_CHOLESKY && J->kind != LSQ_MAT_DENSE && !blockdiag && !bordered) {
        lsq_set_error("MethodError: no AbstractAllocatedSolver for Cholesky() with a sparse Jacobian "
                      "(dense_cholesky.jl:19 requires a StridedVecOrMat)");
        return LSQ_EARG;
    }
    LSQ_HIP(hipSetDevice(c->device));
    lsq_solver *s = new lsq_solver();
    s->ctx = c;
    s->kind = kind;
    s->for_lm = for_lm ? 1 : 0;
    s->m = J->m;
    s->n = J->n;
    int st = (kind == LSQ_LSMR) ? lsq_lsmr_alloc(s) : (kind == LSQ_BLOCK_QR) ? lsq_blockqr_solver_alloc(s, J)
             : (kind == LSQ_SCHUR) ? lsq_schur_solver_alloc(s, J) : (kind == LSQ_BORDERED_QR) ? lsq_borderedqr_solver_alloc(s, J)
             : blockdiag ? lsq_blockdiag_solver_alloc(s, J) : bordered ? lsq_bordered_solver_alloc(s, J) : lsq_dense_solver_alloc(s);
    if (st != LSQ_OK) {
        delete s;
        return st;
    }
    *out = s;
    return LSQ_OK;
}

extern "C" int lsq_solver_destroy(lsq_solver *s) {
    if (!s) return LSQ_OK;
    hipStreamSynchronize(s->ctx->stream);
    if (s->kind == LSQ_LSMR) lsq_lsmr_free(s);
    else lsq_dense_solver_free(s);     // (also the block-diagonal solvers: all they own is d_info, freed there)
    hipFree(s->d_cov_info); hipFree(s->d_cov_buf);     // lsq_solver_covariance
    hipFree(s->d_lev_buf);                             // lsq_dense_qr_leverage / lsq_solver_leverage
    if (s->inner) {                                // lsq_sparse_covariance, Schur(), BorderedQR()
        hipFree(s->inner->d_cov_buf);              // (lsq_bordered_qr_covariance: the inner QR()'s zero right-hand side)
        lsq_dense_solver_free(s->inner);
        delete s->inner;
    }
    delete s->inner_J;                             // (a view: its values belong to d_work)
    delete s;
    return LSQ_OK;
}

// include/lsqhip.h: "calls that return host scalars synchronise the stream".  The LSMR driver learns about the stop from a
// progress word that the committing workgroup publishes BEFORE its sibling workgroups have finished writing x (lsq_lsmr3.h:
// relaxed publish), and launches of the look-ahead may still be queued: the public entry points drain the stream
// before they hand nmul back, so that x may be read from another stream or with a blocking copy.  (Polled, not
// hipStreamSynchronize: what is left in the queue is microseconds of work, a sleeping wait wakes up after ~50 us.)  The LM /
// Dogleg loops call lsq_lsmr_solve directly and stay stream-ordered.
static int lsmr_drain(lsq_solver *s) {
    for (;;) {
        const hipError_t q = hipStreamQuery(s->ctx->stream);
        if (q == hipSuccess) return LSQ_OK;
        if (q != hipErrorNotReady) {
            lsq_set_error("HIP error behind an LSMR solve: %s", hipGetErrorString(q));
            return LSQ_EHIP;
        }
    }
}

extern "C" int lsq_ldiv(lsq_solver *s, lsq_mat *J, const double *y, double *x, int *nmul) {
    LSQ_RANGE("lsq_ldiv");
    if (!s || !J || !y || !x) return LSQ_EARG;
    if (s->for_lm && s->kind == LSQ_QR) {
        lsq_set_error("ldiv!: this QR solver was allocated for LevenbergMarquardt (damped)");
        return LSQ_EDIM;
    }
    switch (s->kind) {
    case LSQ_LSMR: LSQ_TRY(lsq_lsmr_solve(s, J, y, nullptr, x, nmul)); return lsmr_drain(s);
    case LSQ_CHOLESKY:
        if (s->br_blocks) return lsq_bordered_solve(s, J, y, nullptr, x, nmul);     // (refused: LM only)
        return s->bd_blocks ? lsq_blockdiag_solve(s, J, y, nullptr, x, nmul) : lsq_cholesky_solve(s, J, y, nullptr, x, nmul);
    case LSQ_BLOCK_QR: return lsq_blockqr_solve(s, J, y, nullptr, x, nmul);
    case LSQ_SCHUR: return lsq_schur_solve(s, J, y, nullptr, x, nmul);             // (refused: LM only)
    case LSQ_BORDERED_QR: return lsq_borderedqr_solve(s, J, y, nullptr, x, nmul);  // (refused: LM only)
    default: return lsq_qr_solve(s, J, y, nullptr, x, nmul);
    }
}

extern "C" int lsq_ldiv_damped(lsq_solver *s, lsq_mat *J, const double *y, double *damp, double *x, int *nmul) {
    LSQ_RANGE("lsq_ldiv_damped");
    if (!s || !J || !y || !x || !damp) return LSQ_EARG;
    switch (s->kind) {
    case LSQ_LSMR: LSQ_TRY(lsq_lsmr_solve(s, J, y, damp, x, nmul)); return lsmr_drain(s);
    case LSQ_CHOLESKY:
        if (s->br_blocks) return lsq_bordered_solve(s, J, y, damp, x, nmul);
        return s->bd_blocks ? lsq_blockdiag_solve(s, J, y, damp, x, nmul) : lsq_cholesky_solve(s, J, y, damp, x, nmul);
    case LSQ_BLOCK_QR: return lsq_blockqr_solve(s, J, y, damp, x, nmul);
    case LSQ_SCHUR: return lsq_schur_solve(s, J, y, damp, x, nmul);
    case LSQ_BORDERED_QR: return lsq_borderedqr_solve(s, J, y, damp, x, nmul);
    default: return lsq_qr_solve(s, J, y, damp, x, nmul);
    }
}

extern "C" int lsq_solver_set_preconditioner(lsq_solver *s, lsq_precond_callback cb, void *user) {
    if (!s) return LSQ_EARG;
    if (s->kind != LSQ_LSMR && cb) {
        lsq_set_error("preconditioners apply to the LSMR solver only (types.jl:82-86)");
        return LSQ_EARG;
    }
    s->precond_cb = cb;
    s->precond_user = user;
    return LSQ_OK;
}

extern "C" int lsq_solver_qr_panel(const lsq_solver *s, int *kind) {
    if (!s || !kind) { lsq_set_error("lsq_solver_qr_panel: null argument"); return LSQ_EARG; }
    *kind = s->kind == LSQ_BORDERED_QR ? s->inner->last_qr_panel : s->last_qr_panel;   // (BorderedQR(): the inner QR()'s)
    return LSQ_OK;
}
extern "C" int lsq_solver_qr_path(const lsq_solver *s, int *path) {
    if (!s || !path) { lsq_set_error("lsq_solver_qr_path: null argument"); return LSQ_EARG; }
    *path = s->kind == LSQ_BORDERED_QR ? s->inner->last_qr_path : s->last_qr_path;
    return LSQ_OK;
}

extern "C" int lsq_solver_stats(const lsq_solver *s, int h_giveups[4], int h_paused[4]) {
    if (!s) { lsq_set_error("lsq_solver_stats: null argument"); return LSQ_EARG; }
    const LsqFallback *fb[4] = {&s->fb_tiles, &s->fb_pipe, &s->fb_qrx, &s->fb_cholqr};
    for (int i = 0; i < 4; ++i) {
        if (h_giveups) h_giveups[i] = fb[i]->giveups;
        if (h_paused) h_paused[i] = fb[i]->cooldown;
    }
    if (s->kind == LSQ_BORDERED_QR) {      // the inner QR()'s panel exchange and CholeskyQR2 panels
        for (int i = 2; i < 4; ++i) {
            const LsqFallback &fi = i == 2 ? s->inner->fb_qrx : s->inner->fb_cholqr;
            if (h_giveups) h_giveups[i] += fi.giveups;
            if (h_paused) h_paused[i] += fi.cooldown;
        }
    } else if (s->inner) {      // an LSMR() solver after lsq_sparse_covariance, a Schur() solver: the factorisation of its inner dense solver
        if (h_giveups) h_giveups[0] += s->inner->fb_tiles.giveups;
        if (h_paused) h_paused[0] += s->inner->fb_tiles.cooldown;
    }
    return LSQ_OK;
}

extern "C" int lsq_solver_chol_path(const lsq_solver *s, int *path) {
    if (!s || !path) { lsq_set_error("lsq_solver_chol_path: null argument"); return LSQ_EARG; }
    *path = s->inner ? s->inner->last_chol_path : s->last_chol_path;   // (LSMR() after lsq_sparse_covariance, Schur(): the inner solver's factorisation)
    return LSQ_OK;
}

extern "C" int lsq_solver_lsmr_path(const lsq_solver *s, int *path) {
    if (!s || !path) { lsq_set_error("lsq_solver_lsmr_path: null argument"); return LSQ_EARG; }
    *path = s->last_lsmr_path;
    return LSQ_OK;
}

extern "C" int lsq_solver_info(const lsq_solver *s, int *iter, int *istop, int *rank) {
    if (iter) *iter = s->last_iter;
    if (istop) *istop = s->last_istop;
    if (rank) {
        *rank = -1;
        if (s->kind == LSQ_QR && s->d_info) {
            LSQ_HIP(hipStreamSynchronize(s->ctx->stream));
            LSQ_HIP(hipMemcpy(rank, s->d_info, sizeof(int), hipMemcpyDeviceToHost));
        } else if (s->kind == LSQ_BORDERED_QR && s->last_bd_path == 6) {   // the locals have full rank or the solve failed
            int inner_rank = 0;
            LSQ_TRY(lsq_solver_info(s->inner, nullptr, nullptr, &inner_rank));
            *rank = s->br_blocks * s->br_nb + inner_rank;
        } else if (s->kind == LSQ_BLOCK_QR && s->bq_solved) {    // the sum of the block ranks
            std::vector<int> hr((size_t)s->bd_blocks);
            LSQ_TRY(lsq_solver_blockdiag_ranks(s, hr.data()));
            *rank = 0;
            for (int v : hr) *rank += v;
        }
    }
    return LSQ_OK;
}

