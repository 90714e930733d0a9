// AbstractAllocatedSolver equivalents (types.jl:138-139): buffers are allocated once per problem
// (README "minimal allocation"), never inside an iteration.
#pragma once
#include "lsq_common.h"

// Device-resident LSMR recurrence (lsmr.jl:82-113 initial values, :127-196 per-iteration update).
struct LsmrState {
    double alpha, beta, rho, rhobar, cbar, sbar, zeta, zetabar, alphabar;
    double betadd, betad, rhodold, tautildeold, thetatilde, d;
    double normA2, maxrbar, minrbar, normb, normr, normAr, normA, condA, normx;
    // coefficients consumed by the vector kernels
    double cu;        // u~ <- A v - cu * u~        (cu = alpha / beta: u is kept unnormalised)
    double inv_beta;  // v~ <- P (J'u~ + d ux~) * inv_beta - beta * v
    double vscale;    // v  <- v~ * vscale          (1/alpha, or 1 when the v update was skipped)
    double c1, c2, c3;
    double atol, btol, ctol;
    int iter, istop, done, maxiter;
    int beta_zero;    // lsmr.jl:120: beta == 0 skips the v update
    int first;        // setup pass (lsmr.jl:73-78)
    unsigned epoch;
    int notdone;      // !done: the skip flag of launches that were queued to run AFTER the solve (the LM loop's step /
                      // predicted residual / trial residual chain, enqueued behind the predicted last iteration)
};

// A fast path that relies on what the hardware does but HIP does not promise (all workgroups of a launch co-resident and
// dispatched in index order: in-kernel tile / slab exchanges) has bounded waits; a wait that gives up is COUNTED and the path
// is switched off for a while -- not for ever: after `cooldown` further solves it is armed again (a neighbour on the device,
// e.g. an RCCL kernel of a sharded run, may be gone by then); if it gives up again right away the next pause is four times
// as long (16, 64, ... 4096 solves), a clean armed solve resets the pause to 16.
struct LsqFallback {
    int giveups = 0;        // how often a bounded wait of this path gave up (lsq_solver_stats)
    int cooldown = 0;       // solves left before the path is armed again (0: armed)
    int next_pause = 16;
    bool exchange = true;   // false: the path has no in-kernel exchange (fb_cholqr: a numerical fallback) -- LSQ_DEBUG_SERIAL=2 leaves it on
    bool off() const { return cooldown > 0 || (exchange && lsq_dbg_serial >= 2); }
    void gave_up(lsq_ctx *c, int which) {
        giveups++;
        c->fallback_giveups[which]++;
        cooldown = next_pause;
        next_pause = next_pause < 4096 ? next_pause * 4 : 4096;
    }
    void solve_done(bool used_and_clean) {      // once per solve of the owning solver
        if (cooldown > 0) --cooldown;
        else if (used_and_clean) next_pause = 16;
    }
};
enum { LSQ_FB_CHOL_TILES = 0, LSQ_FB_TRI_PIPE = 1, LSQ_FB_QR_EXCHANGE = 2, LSQ_FB_CHOLQR = 3 };

struct lsq_solver {
    lsq_ctx *ctx;
    int kind;
    int for_lm;
    int m, n;
    // --- LSMR (iterative_lsmr.jl:161-171, 216-231) ---
    LsmrState *d_state = nullptr;
    double *d_u = nullptr;     // m
    double *d_ux = nullptr;    // n   (damped rows of u; the reference's `zerosvector`)
    double *d_v = nullptr, *d_h = nullptr, *d_hbar = nullptr, *d_t = nullptr;  // n
    double *d_P = nullptr;     // n   InverseDiagonal._
    double *d_dg = nullptr;    // n   sqrt(damp)
    double *d_red = nullptr;   // deferred-reduction partials: pu[4096] | pv[4096] | int counts[2]
    double *d_f3 = nullptr;    // three-launch iteration (lsq_lsmr3.h): x2 | hbar2 | h2 (n each) | pu[2][4096] | pn[2][3][UB_MAX] | int counts
    size_t f3_elems = 0;
    unsigned f3_tag = 0;       // tag of the newest in-launch record of k_lsmr_fused
    unsigned epoch = 0;
    int last_iter = 0, last_istop = 0;
    int last_lsmr_path = 0;    // lsq_solver_lsmr_path
    // row-sharded single problem (lsq_options.row_allreduce): J is this rank's row block; J'u and sum(u^2) are summed over
    // the ranks in d_xbuf (n + 1 doubles) between the adjoint product and its epilogue
    int (*row_cb)(double *, int, void *, void *) = nullptr;
    void *row_user = nullptr;
    long long global_rows = 0;
    double *d_xbuf = nullptr;  // n + 2
    // colsumabs2 of the WHOLE Jacobian (sum over the ranks of the row blocks' column sums) for the default Jacobi
    // preconditioner and LM's damping: solver-owned, keyed on the handle and its version -- the handle's own cache keeps
    // the LOCAL block's sums, which is what lsq_colsumabs2(J) and any unsharded solve on the same handle must see
    double lsmr_ratio2 = 0.1;     // test2(k) / test2(k-1) as last observed: the starting value of the next solve's stop prediction
    double *d_colsum_g = nullptr;
    unsigned long long colsum_g_uid = 0;     // lsq_mat::uid of the handle the buffer belongs to (0: none)
    unsigned long long colsum_g_version = ~0ull;
    int *d_one = nullptr;      // the constant 1 (partial count of a sum that is already complete)
    // --- dense Cholesky (dense_cholesky.jl:7-21) ---
    double *d_chol = nullptr;  // n*n
    double *d_Ds = nullptr;    // ceil(n/64) factored 64 x 64 diagonal blocks in flight (blocked Cholesky)
    double *d_rhs = nullptr;   // n
    int *d_info = nullptr;
    // --- dense QR (dense_qr.jl:6-28, 50-54) ---
    int last_qr_path = 0;      // lsq_solver_qr_path
    int last_qr_panel = 0;     // lsq_solver_qr_panel
    double *d_qr = nullptr;    // (m [+n]) * n
    double *d_qu = nullptr;    // max(m,n) or m+n
    double *d_tau = nullptr;
    double *d_T = nullptr;     // block reflector factors
    double *d_work = nullptr;
    size_t work_elems = 0;
    std::vector<double> h_R;   // n*n host copy for pivoting / rank decisions
    int last_rank = -1;
    // where the last lsq_qr_solve left its factor (lsq_dense_qr_covariance): the triangle R (reflectors may stand below its
    // diagonal) with its leading dimension, pivots in d_tau; certified path: X = inv(R) as well (Qr2Work::Xinv), else nullptr
    const double *qr_R = nullptr, *qr_X = nullptr;
    int qr_ldr = 0;
    int (*precond_cb)(double *, lsq_mat *, const double *, void *) = nullptr;   // LSMR(preconditioner!, P), diagonal P
    void *precond_user = nullptr;
    // LSMR(preconditioner!, P) with ANY P supporting ldiv! (lsq_lsmr_general.hip): update = preconditioner!(P, x, J, damp),
    // ldiv = ldiv!(out, P, in).  Set => the operator-level LSMR runs instead of the fused one.
    int (*gen_update)(lsq_mat *, const double *, void *) = nullptr;
    int (*gen_ldiv)(double *, const double *, void *) = nullptr;
    void *gen_user = nullptr;
    void *qr2 = nullptr;            // two-stage QR workspace (lsq_dense.hip), allocated on first use
    void (*qr2_free)(void *) = nullptr;
    void *tripipe = nullptr;        // pipelined triangular solves of the blocked Cholesky (lsq_dense.hip)
    void (*tripipe_free)(void *) = nullptr;
    double *tri_X = nullptr, *tri_T = nullptr, *tri_fro = nullptr, *tri_hfro = nullptr;   // explicit inverse of the Cholesky factor (Dogleg certificate)
    int last_chol_path = 0;         // lsq_solver_chol_path
    LsqFallback fb_pipe;            // pipelined triangular solves (else single-workgroup solves)
    bool chol_have_diaginv = false; // the last blocked factorisation left inv(U_kk) in the solve pipeline's buffer
    unsigned *d_chol_flags = nullptr; // k_chol_chain: epoch-tagged 'tile published' flags
    unsigned chol_epoch = 0;
    LsqFallback fb_tiles;           // one-launch factorisation k_chol_chain (else launch-per-panel)
    LsqFallback fb_qrx;             // QR: slab exchange of the panel steps + pipelined certified solve (mirrors Qr2Work::no_exchange)
    LsqFallback fb_cholqr{0, 0, 16, false};   // QR: CholeskyQR2 panels (numerical breakdowns; mirrors Qr2Work::no_cholqr)
    bool last_chol_tiles = false;   // the last blocked factorisation was the one-launch one
    bool pub_want = false;          // lsq_tri_chol_solve: let the backward solve's last block publish {info, pipeline flag}
    unsigned long long pub_seq = 0; // ... sequence number of that hand-over (0: it was not launched, use lsq_read_ints)
    // --- Cholesky() on a block-diagonal Jacobian (lsq_blockdiag.hip): bd_blocks > 0; only d_info is allocated ---
    int bd_blocks = 0, bd_mb = 0, bd_nb = 0;
    int last_bd_path = 0;           // lsq_solver_blockdiag_path
    int last_bd_block = -1;
    // --- BlockQR() on the same handles (lsq_blockqr.hip): d_info holds the bd_blocks ranks of the last solve ---
    bool bq_solved = false;
    // --- Cholesky() on a bordered block-diagonal Jacobian (lsq_bordered.hip): br_blocks > 0; d_info and d_work (the factor rows,
    // the Schur contributions and their partial sums) are allocated ---
    int br_blocks = 0, br_mb = 0, br_nb = 0, br_ng = 0;
    // --- lsq_solver_covariance on either (lsq_cov.hip, lsq_bordered.hip), allocated on first use: the per-block verdicts;
    // bordered: zeros (the damping and right-hand side of the elimination) followed by the ng x ng block of the shared parameters
    // (the same on a BorderedQR() solver: lsq_bordered_qr_covariance, lsq_cov_bordered.hip)
    int *d_cov_info = nullptr;
    double *d_cov_buf = nullptr;
    // --- lsq_dense_qr_leverage / lsq_solver_leverage (lsq_leverage.hip), grown on demand: the quadratic forms q when the
    // caller asks only for what is derived from them; block-diagonal handles: the B variances s_b^2 in front of them;
    // lsq_bordered_qr_leverage (lsq_lev_bordered.hip): ||z||^2 | ||u||^2 | q | for new rows their p x ng matrix E
    double *d_lev_buf = nullptr;
    size_t lev_cap = 0;
    // --- a dense Cholesky() solver (lsq_dense_solver_alloc) owned by this one, factoring a Gram matrix that is written into its
    // d_chol.  lsq_sparse_covariance on an LSMR() solver (lsq_cov_sparse.hip), created on first use: m, n of this one, J'J.
    // Schur() on a bordered handle (lsq_schur.hip; br_blocks > 0, d_info and d_work as above), created with the solver: n = ng,
    // the Schur complement of the locals
    // BorderedQR() on a bordered handle (lsq_borderedqr.hip; br_blocks > 0, d_info and d_work as above), created with the solver:
    // a dense QR() solver (for_lm) with m rows and n = ng, and inner_J, the dense handle it solves on: a view of the
    // transformed border inside d_work that owns nothing
    lsq_solver *inner = nullptr;
    lsq_mat *inner_J = nullptr;
};
int lsq_tri_chol_solve(lsq_solver *s, const double *U, int n, double *d_bx);
int lsq_tri_chol_fwd_operands(lsq_solver *s, int n, double **z, unsigned long long **slot, unsigned long long *epoch, int **err);
// buffer of the inverted 64 x 64 diagonal blocks of the pipelined solves (allocates the pipeline; nullptr when it is off)
double *lsq_tri_chol_diagbuf(lsq_solver *s, int n);

#ifdef __HIPCC__
// the scalar recurrence of one iteration (lsmr.jl:127-196, :205), on a private copy of the state
__device__ inline void lsmr_rotate_inline(LsmrState &s, double alpha, double beta) {
    const double lambda = 0.0;
    // lsmr.jl:127-130
    double alphahat = sqrt(s.alphabar * s.alphabar + lambda * lambda);
    double chat = s.alphabar / alphahat, shat = lambda / alphahat;
    // :132-138
    double rhoold = s.rho;
    double rho = sqrt(alphahat * alphahat + beta * beta);
    double c = alphahat / rho, sn = beta / rho;
    double thetanew = sn * alpha;
    s.alphabar = c * alpha;
    // :140-149
    double rhobarold = s.rhobar, zetaold = s.zeta;
    double thetabar = s.sbar * rho;
    double rhotemp = s.cbar * rho;
    double rhobar = sqrt((s.cbar * rho) * (s.cbar * rho) + thetanew * thetanew);
    s.cbar = s.cbar * rho / rhobar;
    s.sbar = thetanew / rhobar;
    s.zeta = s.cbar * s.zetabar;
    s.zetabar = -s.sbar * s.zetabar;
    s.rho = rho;
    s.rhobar = rhobar;
    // :152-156 coefficients of the vector updates
    s.c1 = -thetabar * rho / (rhoold * rhobarold);
    s.c2 = s.zeta / (rho * rhobar);
    s.c3 = -thetanew / rho;
    // :164-184 estimate of ||r||
    double betaacute = chat * s.betadd, betacheck = -shat * s.betadd;
    double betahat = c * betaacute;
    s.betadd = -sn * betaacute;
    double thetatildeold = s.thetatilde;
    double rhotildeold = sqrt(s.rhodold * s.rhodold + thetabar * thetabar);
    double ctildeold = s.rhodold / rhotildeold, stildeold = thetabar / rhotildeold;
    s.thetatilde = stildeold * rhobar;
    s.rhodold = ctildeold * rhobar;
    s.betad = -stildeold * s.betad + ctildeold * betahat;
    s.tautildeold = (zetaold - thetatildeold * s.tautildeold) / rhotildeold;
    double taud = (s.zeta - s.thetatilde * s.tautildeold) / s.rhodold;
    s.d = s.d + betacheck * betacheck;
    s.normr = sqrt(s.d + (s.betad - taud) * (s.betad - taud) + s.betadd * s.betadd);
    // :187-189 ||A||
    s.normA2 = s.normA2 + beta * beta;
    s.normA = sqrt(s.normA2);
    s.normA2 = s.normA2 + alpha * alpha;
    // :192-196 cond(A)
    s.maxrbar = fmax(s.maxrbar, rhobarold);
    if (s.iter + 1 > 1) s.minrbar = fmin(s.minrbar, rhobarold);
    s.condA = fmax(s.maxrbar, rhotemp) / fmin(s.minrbar, rhotemp);
    s.normAr = fabs(s.zetabar);                      // :205
}

#endif

// implemented in lsq_lsmr.hip
int lsq_lsmr_alloc(lsq_solver *s);
void lsq_lsmr_free(lsq_solver *s);
// d_Jty (optional): J'*y already formed by the caller (the LM gradient) -- skips the setup product;
// y_sumsq (optional, < 0 = unknown): sum(y.^2) when the caller already holds it (the LM loop's ssr)
// lm (optional, with d_Jty and y_sumsq): the LM loop's damping and projected gradient norm (levenberg_marquardt.jl:82-86,
// 102-104) are formed by the solve's own setup launch -- d_damp is then an OUTPUT (dtd/Delta, left as its square root like
// after every damped solve) and *lm->out_grad receives max|g| -- instead of a launch of their own in front of it
struct LsmrLmPrep {
    const double *colsum;     // colsumabs2(J)
    double inv_delta, min_diag, max_diag;
    const double *x, *lo, *hi;
    double *out_grad;
};
constexpr int LSMR_LM_PREP_MAX_N = 16384;   // every workgroup of that launch reduces colsum and g over all n itself
// tail (optional): what the caller will launch once the solve is over and which depends on nothing but d_x.  `predict` > 0: a
// guess at the solve's last inner iteration (the inner count of an LM run changes slowly).  The three-launch iteration
// (lsmr_run_fused) REACTS: the launch that commits the guessed iteration is cautious, nothing is queued behind it until it has
// reported, and the tail is called once, with skip = nullptr, after the stop has been seen.  The four-launch iteration
// (lsmr_run_four) PRE-PLACES: the tail is enqueued right behind inner iteration `predict` with skip = &state->notdone (its
// kernels return at once if the solve is NOT over by then) and no further iteration is queued until that one has reported; a
// tail that skipped itself may be queued again, guarded, behind a later iteration, and unless a guarded tail is known to have
// run the tail is called (again) with skip = nullptr after the solve.  predict == 0, general preconditioner, reference-order
// kernels: called once after the solve.  `dynamic`: from inner iteration 1 on the guess is replaced by a prediction from the
// hints beside the progress word (StopPredictor, lsq_lsmr.hip).
// `step` (optional; plain device pointers): the tail BEGINS with the LM loop's step x_trial = x - d_x (k_step: with tanh and
// 1 - tanh^2 of x_trial where t_out is set, max|d_x| -> *out_dx, the first non-finite index of x_trial -> *out_nonfin through one
// ticket round on partials / counter).  The three-launch iteration then queues k_lsmr_commit_step (lsq_lsmr3.h) where it would
// queue a cautious launch: if that launch finds the solve over it has taken the step itself and *step_taken is set before the
// tail is called -- the tail then leaves its step kernel out.  A stop that an ordinary launch commits, every other driver and
// LSQ_NO_COMMIT_STEP=1 leave *step_taken clear.
struct LsmrStepDesc {
    const double *x = nullptr;
    double *xt = nullptr, *t_out = nullptr, *s_out = nullptr;
    double *partials = nullptr;
    unsigned *counter = nullptr;
    double *out_dx = nullptr, *out_nonfin = nullptr;
};
struct LsmrTail {
    int predict = 0;
    int (*fn)(const int *skip, void *user) = nullptr;
    void *user = nullptr;
    bool dynamic = false;
    const LsmrStepDesc *step = nullptr;
    bool *step_taken = nullptr;
};
int lsq_rowshard_colsum(lsq_solver *s, lsq_mat *J, const double **out);   // colsumabs2 of the whole J (row-sharded: summed over the ranks)
int lsq_lsmr_solve(lsq_solver *s, lsq_mat *J, const double *d_y, double *d_damp, double *d_x, int *nmul,
                   const double *d_Jty = nullptr, double y_sumsq = -1.0, const LsmrLmPrep *lm = nullptr,
                   const LsmrTail *tail = nullptr);
// whether lsq_lsmr_solve takes the LsmrLmPrep route for this solver / Jacobian (else the caller launches its own damping)
bool lsq_lsmr_takes_lm_prep(const lsq_solver *s, const lsq_mat *J);
// implemented in lsq_lsmr_general.hip (operator-level LSMR around a caller-supplied ldiv!(., P, .))
int lsq_lsmr_general_solve(lsq_solver *s, lsq_mat *J, const double *d_y, double *d_damp, double *d_x, int *nmul);
// implemented in lsq_exact.hip (reference-order kernels for small problems)
int lsq_lsmr_exact_solve(lsq_solver *s, lsq_mat *J, const double *d_y, double *d_damp, double *d_x, int *nmul);
// implemented in lsq_dense.hip
int lsq_dense_solver_alloc(lsq_solver *s);
void lsq_dense_solver_free(lsq_solver *s);
int lsq_cholesky_solve(lsq_solver *s, lsq_mat *J, const double *d_y, const double *d_damp, double *d_x, int *nmul);
int lsq_qr_solve(lsq_solver *s, lsq_mat *J, const double *d_y, const double *d_damp, double *d_x, int *nmul);
bool lsq_cholesky_takes_blocked(int m, int n);
int lsq_cholesky_small_factor(lsq_solver *s, lsq_mat *J);
int lsq_cholesky_small_factor_ready(lsq_solver *s, int n);
// implemented in lsq_qr.hip: X = inv(U) into the upper triangle of s->tri_X (stream-ordered; tri_X / tri_T allocated on first use)
int lsq_tri_inv_enqueue(lsq_solver *s, const double *U, int n);
// implemented in lsq_blockdiag.hip
int lsq_blockdiag_solver_alloc(lsq_solver *s, const lsq_mat *J);
int lsq_blockdiag_solve(lsq_solver *s, lsq_mat *J, const double *d_y, const double *d_damp, double *d_x, int *nmul);
int lsq_blockdiag_solve_blocks(lsq_ctx *c, lsq_mat *J, bool pivot, const double *d_y, const double *d_delta, double *d_x,
                               const int *d_active, int *d_binfo, double *d_r, double *d_diag);
// implemented in lsq_bordered.hip
int lsq_bordered_solver_alloc(lsq_solver *s, const lsq_mat *J);
int lsq_bordered_solve(lsq_solver *s, lsq_mat *J, const double *d_y, const double *d_damp, double *d_x, int *nmul);
int lsq_bordered_covariance(lsq_solver *s, lsq_mat *J, const double *d_f, double *d_cov, double *d_stderr, int *h_info);
// implemented in lsq_schur.hip
int lsq_schur_solver_alloc(lsq_solver *s, const lsq_mat *J);
int lsq_schur_solve(lsq_solver *s, lsq_mat *J, const double *d_y, const double *d_damp, double *d_x, int *nmul);
// implemented in lsq_borderedqr.hip
int lsq_borderedqr_solver_alloc(lsq_solver *s, const lsq_mat *J);
int lsq_borderedqr_solve(lsq_solver *s, lsq_mat *J, const double *d_y, const double *d_damp, double *d_x, int *nmul);
// implemented in lsq_cov_dense.hip: lsq_dense_qr_covariance in front of and behind its wait for the rank (s->d_info[0])
int lsq_dense_qr_cov_factor(lsq_solver *s, lsq_mat *J, const double **X, const int **jp);
int lsq_dense_qr_cov_finish(lsq_solver *s, int n, const double *X, const int *jp, double s2, double *d_cov, double *d_stderr);
struct LsqBdqView { double *R, *W, *F; };     // R_b (B nb x nb, rows) | W ((B nb) x ng, column-major) | F ((B mb) x ng) in d_work
int lsq_borderedqr_eliminate(lsq_solver *s, lsq_mat *J, const double *d_y, const double *d_damp, LsqBdqView *view);
// implemented in lsq_leverage.hip: the solver's leverage scratch (d_lev_buf), grown to `doubles`; the hot path and the derived
// outputs of lsq_dense_qr_leverage, which lsq_bordered_qr_leverage (lsq_lev_bordered.hip) launches on its own operands
int lsq_lev_scratch(lsq_solver *s, size_t doubles, double **out);
#ifdef __HIPCC__
__global__ void k_lev_tall(const double *__restrict__ A, int lda, int p, int n, const double *__restrict__ X,
                           const int *__restrict__ jp, const double *__restrict__ scale, double *__restrict__ q);
__global__ void k_lev_diag(long long m, const double *__restrict__ q, const double *__restrict__ f, double s2,
                           const double *__restrict__ s2b, int mb, double ncook, double *__restrict__ se, double *__restrict__ t,
                           double *__restrict__ cook);
#endif
// implemented in lsq_blockqr.hip
int lsq_blockqr_solver_alloc(lsq_solver *s, const lsq_mat *J);
int lsq_blockqr_solve(lsq_solver *s, lsq_mat *J, const double *d_y, const double *d_damp, double *d_x, int *nmul);
int lsq_blockqr_solve_blocks(lsq_ctx *c, lsq_mat *J, bool lm, const double *d_y, const double *d_delta, double *d_x,
                             const int *d_active, int *d_ranks, double *d_r, double *d_diag);
// implemented in lsq_optimize.hip: g!(J, x) with the handle's bookkeeping around it (version, mirrors)
int lsq_call_g(lsq_g_callback g, lsq_mat *J, const double *x, void *user);
