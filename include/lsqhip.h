/*
 * lsqhip.h -- C ABI of the MI355X (gfx950) nonlinear-least-squares hot path.
 *
 * This is the drop-in boundary for LeastSquaresOptim.jl's linear-algebra inner loop.  The reference
 * has no FFI layer: its plug points are Julia multiple dispatch on AbstractAllocatedSolver and a
 * duck-typed operator interface.  Every entry point below names the reference interface it
 * replaces (file:line relative to the reference repo); INTEGRATION.md shows the `ccall` shim a
 * maintainer would add on the Julia side.
 *
 * Conventions: plain pointers and sizes only; `double*` arguments named d_* are DEVICE pointers
 * (fp64), h_* are host pointers; matrices are column-major; indices are 0-based int32; every call
 * returns an lsq_status (0 = ok) and never aborts; lsq_last_error() gives the message.
 * All work is enqueued on the context's HIP stream; calls that return host scalars synchronise it.
 */
#ifndef LSQHIP_H
#define LSQHIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    LSQ_OK = 0,
    LSQ_EDIM = 1,       /* DimensionMismatch / ArgumentError (types.jl:14-15, dense_qr.jl:10,61) */
    LSQ_ENOTPD = 2,     /* PosDefException from cholesky! (dense_cholesky.jl:57) */
    LSQ_ERANK = 3,      /* RankDeficientException from pivoted cholesky! (dense_cholesky.jl:33) */
    LSQ_ENONFINITE = 4, /* IsFiniteException (utils.jl:63-75) */
    LSQ_EBOUNDS = 5,    /* "Initial guess must be within bounds" (levenberg_marquardt.jl:51) */
    LSQ_EHIP = 6,       /* a HIP runtime call failed */
    LSQ_EARG = 7,       /* invalid argument (e.g. QR on a sparse Jacobian, types.jl:115-117) */
    LSQ_ECALLBACK = 8,  /* a user callback reported failure */
    LSQ_ERCCL = 9       /* sharded run: the exchange reported that a peer rank left its loop with an error */
} lsq_status;

typedef struct lsq_ctx lsq_ctx;       /* one per device/stream; not thread-safe */
typedef struct lsq_mat lsq_mat;       /* Jacobian: dense column-major or CSC (+CSR mirror) */
typedef struct lsq_solver lsq_solver; /* AbstractAllocatedSolver (types.jl:138-139) */
typedef struct lsq_model lsq_model;   /* built-in device-side f!/g! (synthetic benchmarks) */

/* types.jl:79-86; LSQ_BLOCK_QR: QR() per block of a block-diagonal handle (lsq_blockdiag_create), one rank decision per block;
 * LSQ_SCHUR: Cholesky()'s damped solve on a bordered handle (lsq_blockdiag_bordered_create) with any number of shared columns */
typedef enum { LSQ_QR = 0, LSQ_CHOLESKY = 1, LSQ_LSMR = 2, LSQ_BLOCK_QR = 3, LSQ_SCHUR = 4 } lsq_solver_kind;
/* one more solver kind (lsq_solver_create and lsq_optimize take the kind as an int): the backward-stable direct solver on a
 * bordered handle, Householder QR of the locals block by block and a dense QR() of what is left of the border */
enum { LSQ_BORDERED_QR = 5 };
typedef enum { LSQ_DOGLEG = 0, LSQ_LEVENBERG_MARQUARDT = 1 } lsq_optimizer_kind;   /* types.jl:90-98 */

const char *lsq_last_error(void);
int lsq_version(void);

/* ---- context & raw device memory (Julia GC owns nothing here; explicit create/destroy) ---- */
int lsq_ctx_create(int device, void *hip_stream_or_null, lsq_ctx **out);
int lsq_ctx_destroy(lsq_ctx *ctx);
int lsq_ctx_sync(lsq_ctx *ctx);
void *lsq_ctx_stream(lsq_ctx *ctx);
int lsq_malloc(lsq_ctx *ctx, size_t bytes, void **d_out);
int lsq_free(lsq_ctx *ctx, void *d_ptr);
int lsq_h2d(lsq_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int lsq_d2h(lsq_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
int lsq_d2d(lsq_ctx *ctx, void *d_dst, const void *d_src, size_t bytes);
/* page-locked host memory: what a host-side g! should write the Jacobian values into, so that the upload after every
 * g!(J, x) (levenberg_marquardt.jl:77-81: 80 MB at C4) runs at the PCIe rate, asynchronously (lsq_mat_set_values_async) */
int lsq_host_alloc(lsq_ctx *ctx, size_t bytes, void **h_out);
int lsq_host_free(lsq_ctx *ctx, void *h_ptr);

/* ---- Jacobian handles ---- */
/* Dense m x n, column-major, device-owned (the `J::Matrix` of types.jl:36). */
int lsq_dense_create(lsq_ctx *ctx, int m, int n, lsq_mat **out);
/* CSC pattern given once (SparseMatrixCSC with a FIXED pattern, as the reference's sparse g!
 * requires: test/nonlinearleastsquares.jl:47-86).  Builds the CSR mirror + CSC->CSR value map. */
int lsq_csc_create(lsq_ctx *ctx, int m, int n, const int *h_colptr, const int *h_rowval, lsq_mat **out);
/* J = blkdiag(J_1 .. J_B), every block dense mb x nb: m = B*mb, n = B*nb.  Values are addressed exactly like a CSC
 * handle with that pattern: nzval order = [block][column][row], i.e. B column-major mb x nb blocks back to back
 * (lsq_mat_set_values / _async / lsq_mat_values / lsq_mat_get_values / lsq_mat_refresh / lsq_mat_set_colscale).  The handle
 * IS a CSC handle (products, column sums, LSMR(), column scaling, sharding: unchanged) that also knows its block shape:
 * lsq_solver_create accepts it with LSQ_CHOLESKY when nb <= 64 -- J'J + diag(damp) is block-diagonal, so the normal
 * equations of LevenbergMarquardt(Cholesky()) / Dogleg(Cholesky()) are B independent nb x nb factorisations, one pass over
 * the values per solve, with the reference's semantics on the stacked system (one trust region, LSQ_ENOTPD at the column
 * where the stacked dpotrf stops, LSQ_ERANK when the stacked pivoted factorisation stops early).  LSQ_QR stays refused.
 * LSQ_BLOCK_QR (nb <= 64; any other handle, or nb > 64: LSQ_EARG) is the backward-stable direct solver on such a handle:
 * per block b the reference's QR() on that block alone (dense_qr.jl:30-88) -- x_b = ldiv!(qr!(J_b, ColumnNorm()), y_b) with
 * xGELSY's rank decision at rcond = min(mb, nb) eps; damped: the same on [J_b; diag(sqrt(damp_b))] with right-hand side
 * (y_b, 0) and rcond = nb eps.  The Gram matrix is never formed; a rank-deficient, an all-zero (x_b = 0) or a wide block
 * (mb < nb) gets its minimum-norm solution and is never an error.  nmul is 1, damp is left as it is, a column-scaled handle
 * means J_b S_b.  lsq_ldiv, lsq_ldiv_damped, lsq_optimize (one trust region over the stacked problem) and
 * lsq_optimize_batched take it. */
int lsq_blockdiag_create(lsq_ctx *ctx, int nblocks, int mb, int nb, lsq_mat **out);
/* 0 blocks for any other handle */
int lsq_mat_blockdiag_info(const lsq_mat *J, int *nblocks, int *mb, int *nb);
/* J = [blkdiag(J_1 .. J_B) | C], the Jacobian of a GLOBAL fit: every data set b has its own nb local parameters (J_b dense
 * mb x nb) and ng parameters are shared by all of them (C dense, (B*mb) x ng): m = B*mb, n = B*nb + ng.  Columns 0 .. B*nb-1
 * are the block columns exactly as in lsq_blockdiag_create, columns B*nb .. n-1 the border, each with all m rows.  Values are
 * addressed like a CSC handle with that pattern: nzval order = B column-major mb x nb blocks back to back, then ng columns of
 * m doubles.  The handle IS a CSC handle (products, column sums, LSMR(), column scaling, value upload / refresh, sharding:
 * unchanged) that also knows its shape.  lsq_mat_blockdiag_info answers "0 blocks" for it: the shared columns couple the
 * blocks, so LSQ_BLOCK_QR, lsq_optimize_batched and the per-block Cholesky() refuse it like any other CSC handle.
 * lsq_solver_create accepts it with LSQ_CHOLESKY and for_lm = 1 when nb + ng <= 64 (else LSQ_EARG): J'J + diag(damp) is an
 * arrowhead, with the locals ordered first its Cholesky factor has no fill, and eliminating the locals block by block, then
 * factoring the ng x ng Schur complement IS right-looking dpotrf on the stacked matrix -- so lsq_ldiv_damped and lsq_optimize
 * with LSQ_LEVENBERG_MARQUARDT keep the reference's semantics (dense_cholesky.jl:43-59: one trust region, LSQ_ENOTPD with the
 * 1-based column at which the stacked factorisation stops) at the cost of one pass over the values.  nmul is 1, damp is
 * left as it is, a column-scaled handle means J S.  for_lm = 0 and lsq_ldiv (Dogleg(Cholesky())) are refused with LSQ_EARG on
 * purpose: the reference factors with diagonal pivoting over the whole stacked matrix (dense_cholesky.jl:29-35) and reports
 * RankDeficientException(rank) along that global pivot order, which does not split into "locals first".  LSQ_QR stays
 * refused.  Any of the four sizes < 1, or sizes past 32-bit indices: LSQ_EDIM.
 * LSQ_SCHUR is the same solve without the limit on the border: lsq_solver_create accepts the handle with for_lm = 1 when
 * nb <= 64, for ANY ng >= 1 (memory is the only cap: B*nb*ng doubles for the eliminated border rows, ng*ng for the Schur
 * complement, and the split-K partials of two ng x ng products).  The locals are eliminated block by block in LDS, the border
 * passes through in tiles of 64 columns, and the Schur complement S = C'C + D_g - W'W is factored by the dense Cholesky()
 * machinery on an inner solver.  Semantics are those of LSQ_CHOLESKY on this handle, to the letter: the solution of
 * (J'J + diag(damp)) x = J'y as unpivoted dpotrf on the stacked matrix with the locals first, nmul = 1, damp is not written, a
 * column-scaled handle means J S, one trust region, LSQ_ENOTPD with the 1-based stacked column (b*nb + k in a local block,
 * B*nb + k in the factor of S; the lowest wins) and the message "PosDefException: ... Cholesky failed at <column>"; the solver
 * stays usable afterwards.  lsq_ldiv_damped and lsq_optimize with LSQ_LEVENBERG_MARQUARDT take it (g = NULL included);
 * lsq_solver_blockdiag_path reports 5 (block as for 4), lsq_solver_chol_path the factorisation that took S (1, 2 or 4), and
 * lsq_solver_stats index 0 counts a give-up of its one-launch form (S is then formed again and factored by panel launches).
 * LSQ_EARG: any other handle (dense, plain CSC, block-diagonal, operator), nb > 64, for_lm = 0 / lsq_ldiv / Dogleg (the text
 * of LSQ_CHOLESKY's refusal, for the same reason), lsq_optimize_batched, lsq_solver_covariance (lsq_sparse_covariance on an
 * LSMR() solver serves the handle), a handle of another shape than the solver was created for.
 * LSQ_BORDERED_QR is the backward-stable direct solver on this handle (for_lm = 1, nb <= 64, ANY ng >= 1 and mb >= 1; memory:
 * a copy of the values for the reflectors and the transformed border, B*nb*ng doubles for the triangle's border rows, and
 * the inner QR()'s (m + ng)*ng): lsq_ldiv_damped returns the minimiser of || [J S; diag(sqrt(damp))] x - [y; 0] ||_2 (S: the
 * handle's column scale, if set) by Householder reflectors -- neither J'J nor any part of it is formed, so the solve pays
 * cond(J) where LSQ_CHOLESKY and LSQ_SCHUR pay cond(J)^2.  Per block the rows of [J_b C_b y_b] are eliminated against a
 * triangle that starts as diag(sqrt(damp_b)), the locals unpivoted (Householder QR is columnwise backward stable without
 * pivoting); the transformed border rows, a dense (B*mb) x ng matrix, go with the last ng damping values to ONE damped solve
 * of a dense LSQ_QR solver this one owns; then x_b = inv(R_b) (z_b - W_b x_g).  nmul = 1, damp is not written, stream
 * order, no floating-point atomics.  A diagonal entry of some R_b that is exactly zero or not finite -- possible only where
 * a damping value is zero or an operand is not finite -- is LSQ_ERANK, the message names the 1-based stacked column
 * b*nb + k, the lowest one wins, and the solver stays usable; the shared part follows LSQ_QR's rules (a rank decision, the
 * minimum-norm solution) and never fails on rank.  lsq_ldiv_damped and lsq_optimize with LSQ_LEVENBERG_MARQUARDT take it
 * (bounds and g = NULL included; LM's damping is at least MIN_DIAGONAL * mean(dtd) > 0, so a fit on finite values cannot
 * reach LSQ_ERANK).  lsq_solver_info reports qr_rank = B*nb + the inner rank, lsq_solver_blockdiag_path 6 (after LSQ_ERANK
 * the block), lsq_solver_qr_path / lsq_solver_qr_panel the inner solver's values, lsq_solver_stats (indices 2 and 3) its
 * give-ups.  LSQ_EARG: any other handle, nb > 64, for_lm = 0 / lsq_ldiv / Dogleg (LSQ_CHOLESKY's text, for the same reason),
 * lsq_optimize_batched, lsq_solver_covariance / lsq_dense_covariance / lsq_dense_qr_covariance / lsq_sparse_covariance, a
 * handle of another shape than the solver was created for.  Its covariance, cross-covariances included, is
 * lsq_bordered_qr_covariance below. */
int lsq_blockdiag_bordered_create(lsq_ctx *ctx, int nblocks, int mb, int nb, int ng, lsq_mat **out);
/* all 0 for any other handle */
int lsq_mat_bordered_info(const lsq_mat *J, int *nblocks, int *mb, int *nb, int *ng);
int lsq_mat_destroy(lsq_mat *J);
int lsq_mat_size(const lsq_mat *J, int *m, int *n, long long *nnz);
/* Upload values after a host-side g!(J, x): dense m*n column-major, or nzval in CSC order. */
int lsq_mat_set_values(lsq_mat *J, const double *h_values);
int lsq_mat_get_values(const lsq_mat *J, double *h_values);
/* The same upload without blocking the host: the copy is queued on the context's copy stream (the compute stream keeps
 * running whatever was queued before) and every later use of J on the compute stream waits for it on the DEVICE.
 * h_values must be page-locked (lsq_host_alloc) and must not be written again before lsq_mat_upload_wait(J) returns
 * (or the next call that reads results back has returned).  Pageable memory is accepted and falls back to the
 * synchronous path. */
int lsq_mat_set_values_async(lsq_mat *J, const double *h_pinned_values);
int lsq_mat_upload_wait(lsq_mat *J);
/* Device pointer to the values a device-side g! writes (dense buffer / CSC nzval) ... */
double *lsq_mat_values(lsq_mat *J);
/* ... after which the CSR mirror must be refreshed (no-op for dense).
 * FRESHNESS CONTRACT.  A handle keeps its values in several layouts (CSC order, row and column mirrors or sliced layouts, the
 * stored V of a multiplied-out column scale, the dense buffer), and which of them is the authority changes with the last
 * mutation.  What a caller may rely on: after ANY entry of this header that changes the values -- lsq_mat_set_values / _async,
 * lsq_mat_values + writes + lsq_mat_refresh, lsq_mat_set_colscale / lsq_mat_colscale_changed, lsq_mat_scale_rows,
 * lsq_fd_jacobian, the g! of lsq_model_g and of lsq_loss_g -- every reader (lsq_mat_get_values, lsq_mul, lsq_colsumabs2, lsq_rowsumabs2, lsq_ldiv*, lsq_sparse_gram, the
 * covariance entries, the loops) sees those values and nothing older, in whatever order mutations and readers are mixed, and
 * gives the bits it gives on a freshly created handle holding the same V and s.
 * lsq_mat_values returns the values as they are at that moment; the pointer is for writing until the next entry that changes
 * the values through another route (a g! of lsq_model_g in particular may write the mirrors only): take it again after that.
 * lsq_mat_refresh first brings the CSC-ordered copy up to date with such a g!, then takes it as the authority: called with
 * nothing written it changes no value (so does lsq_mat_set_colscale(J, NULL) on a handle that has no scale). */
int lsq_mat_refresh(lsq_mat *J);
/* J <- diag(w) J: stored entry (i, j) becomes fl(v * w_i), one product; d_w: m device doubles, read during the call's launches.
 * A mutation under the freshness contract: the CSC-ordered copy is made current first (a g! of lsq_model_g may have written
 * the mirrors only), scaled in place -- one read and one write per stored value; a plain CSC handle also reads its row
 * indices, block-diagonal and bordered handles get the row from the position -- and then taken as the authority exactly as by
 * lsq_mat_refresh, so every mirror, sliced layout and windowed copy holds the scaled values.  Behind lsq_mat_set_values_async
 * the scaling waits for the copy on the device.  Stream-ordered, no atomics, no host wait; 0, negative, NaN factors are taken
 * as they are.  LSQ_EARG, with the reason in lsq_last_error: an operator handle (no stored values), a handle with a column scale
 * set (its stored values are V: they would keep every factor while a g! only changes s), a null argument. */
int lsq_mat_scale_rows(lsq_mat *J, const double *d_w);
/* Which layouts the handle has built and which mode it is in (host code: launches nothing, waits for nothing, changes nothing):
 * h_out[0] kind (0 dense, 1 CSC -- block-diagonal and bordered handles included --, 2 operator); [1] sliced rows built (J*x),
 * [2] their column windows, [3] output rows per block; [4] sliced columns built (J'y), [5] their gather windows, [6] column
 * blocks per gather window; [7] windows of the window-blocked CSC (0: not built); [8] / [9] launch plan of the row / column
 * segments (0 stream, 1 wave, 2 block; -1 for a handle that is not CSC); [10] column scale: 0 none, 1 fused (read inside the
 * kernels), 2 multiplied out; [11] 1 when the CSC-ordered copy is current, 0 after a g! that wrote the mirrors only. */
int lsq_mat_layout(const lsq_mat *J, int h_out[12]);

/* ---- column-scaled Jacobians J = V diag(s) ----
 * Models of the form r(x) = V phi(x) - b (phi elementwise) have J(x) = V diag(phi'(x)): the pattern AND the stored values V
 * are fixed, only n factors change from one g!(J, x) to the next (test/nonlinearleastsquares.jl:47-86 is the general case,
 * where g! rewrites nonzeros(J); this is the structured special case).  lsq_mat_set_colscale(J, d_s) declares the values J
 * holds at that moment (lsq_mat_set_values / lsq_mat_values) to be V and d_s (n device doubles, owned by the caller, read
 * whenever J is used) to be s; every operation on the handle -- lsq_mul, lsq_colsumabs2, lsq_rowsumabs2, lsq_ldiv*,
 * lsq_optimize -- then acts on V diag(s).  On the sliced layouts of big sparse patterns nothing is multiplied out: J*x
 * gathers s.*x, J'y = s.*(V'y), colsumabs2(J) = s.^2 .* colsumabs2(V) (cached): a g! costs an n-vector instead of two passes
 * over nnz values.  Other matrices (small, dense, segment-kernel patterns) keep V aside and multiply the values out each
 * time.  A g! that changed s calls lsq_mat_colscale_changed(J) (instead of lsq_mat_refresh); lsq_mat_set_values /
 * lsq_mat_values / lsq_mat_get_values keep addressing V.  d_s = NULL turns J back into the plain matrix V.
 * Entry (i,j) of J is used as V_ij * s_j formed on the fly where the reference would have stored fl(V_ij s_j): results agree
 * with a multiplied-out J to a few ulp per product, not bit for bit (tests/test_a_gpu_contract.py::test_column_scaled_jacobian). */
int lsq_mat_set_colscale(lsq_mat *J, const double *d_s);
int lsq_mat_colscale_changed(lsq_mat *J);

/* ---- custom Jacobian operators (README.md:37-47: any type with mul!, mul! of the adjoint, colsumabs2!,
 *      size, eltype works with LSMR) ----
 * A matrix-free handle: `mul(trans, d_x, d_out, user)` must write J*x (trans = 0, m entries) or J'*x
 * (trans = 1, n entries) into d_out; `colsumabs2(d_out, user)` the n column sums of squares.  Both
 * are HOST callbacks operating on device pointers; the library drains its stream before calling and
 * the callback must have finished its device work when it returns (slow path, like any host-defined
 * operator in the reference).  All fusions of the solvers still apply: the library runs its epilogue
 * over the vector the callback produced.  Works with LSMR (ldiv, lsq_optimize); QR / Cholesky need
 * the entries and refuse it. */
typedef int (*lsq_op_mul_callback)(int trans, const double *d_x, double *d_out, void *user);
typedef int (*lsq_op_colsum_callback)(double *d_out, void *user);
int lsq_op_create(lsq_ctx *ctx, int m, int n, lsq_op_mul_callback mul, lsq_op_colsum_callback colsumabs2,
                  void *user, lsq_mat **out);

/* ---- operator interface (README.md:37-47; used at lsmr.jl:73,76,118,122 and by the optimizers) ---- */
/* mul!(y, J, x, alpha, beta) / mul!(x, J', y, alpha, beta): trans = 0 / 1.
 * Replaces SparseArrays/BLAS mul! at levenberg_marquardt.jl:102,114; dogleg.jl:99,109,171;
 * iterative_lsmr.jl:32,40,91,106. */
int lsq_mul(lsq_mat *J, int trans, double alpha, const double *d_x, double beta, double *d_y);
/* colsumabs2!(out, J): utils.jl:139-151 */
int lsq_colsumabs2(lsq_mat *J, double *d_out);
/* rowsumabs2!(out, J) = colsumabs2!(out, J') for adjoint Jacobians: utils.jl:153-161 (out has m entries) */
int lsq_rowsumabs2(lsq_mat *J, double *d_out);

/* BLAS-1 on device vectors (what lsmr.jl:30-44 and the optimizer loops need from a vector type) */
int lsq_axpy(lsq_ctx *ctx, int n, double a, const double *d_x, double *d_y);       /* axpy!   */
int lsq_scal(lsq_ctx *ctx, int n, double a, double *d_x);                          /* rmul!   */
int lsq_copy(lsq_ctx *ctx, int n, const double *d_x, double *d_y);                 /* copyto! */
int lsq_fill(lsq_ctx *ctx, int n, double a, double *d_x);                          /* fill!   */
int lsq_sumsq(lsq_ctx *ctx, int n, const double *d_x, double *h_out);              /* sum(abs2, x) */
int lsq_sum(lsq_ctx *ctx, int n, const double *d_x, double *h_out);                /* sum(x)  */
int lsq_dot(lsq_ctx *ctx, int n, const double *d_x, const double *d_y, double *h_out);   /* dot(x, y) */
int lsq_emul(lsq_ctx *ctx, int n, const double *d_x, const double *d_y, double *d_out);  /* map!(*, out, x, y): iterative_lsmr.jl:121 */
int lsq_nrm2(lsq_ctx *ctx, int n, const double *d_x, double *h_out);               /* norm(x) */
int lsq_wdot(lsq_ctx *ctx, int n, const double *d_x, const double *d_y, const double *d_w,
             double *h_out);                                                       /* utils.jl:165-175 */
int lsq_amax(lsq_ctx *ctx, int n, const double *d_x, double *h_out);               /* maximum(abs, x) */
/* maxabs_projected_gradient (utils.jl:39-55); d_lower / d_upper may be NULL */
int lsq_amax_projected(lsq_ctx *ctx, int n, const double *d_g, const double *d_x,
                       const double *d_lower, const double *d_upper, double *h_out);
int lsq_clamp(lsq_ctx *ctx, int n, double lo, double hi, double *d_x);             /* clamp!  */
int lsq_ediv(lsq_ctx *ctx, int n, const double *d_x, const double *d_y, double *d_out); /* map!(/, ..) */
/* box step clipping dx = min(dx, x-lower), dx = max(dx, x-upper) (levenberg_marquardt.jl:89-98) */
int lsq_box_clip(lsq_ctx *ctx, int n, double *d_dx, const double *d_x, const double *d_lower,
                 const double *d_upper);
/* first non-finite index or -1 (check_isfinite, utils.jl:70-75) */
int lsq_first_nonfinite(lsq_ctx *ctx, int n, const double *d_x, int *h_index);

/* ---- linear least-squares solvers: THE plug point ---- */
/* AbstractAllocatedSolver(nls, optimizer): dense_qr.jl:25-28,50-54; dense_cholesky.jl:19-21;
 * iterative_lsmr.jl:173-177,233-236.  `for_lm` selects the damped (LevenbergMarquardt) flavour. */
int lsq_solver_create(lsq_ctx *ctx, lsq_mat *J, int solver_kind, int for_lm, lsq_solver **out);
int lsq_solver_destroy(lsq_solver *s);
/* ldiv!(x, J, y, A) -> (x, nmul)       Dogleg: dense_qr.jl:30, dense_cholesky.jl:29,
 *                                              iterative_lsmr.jl:179.  y is preserved. */
int lsq_ldiv(lsq_solver *s, lsq_mat *J, const double *d_y, double *d_x, int *nmul);
/* ldiv!(x, J, y, damp, A) -> (x, nmul) LM: dense_qr.jl:56, dense_cholesky.jl:43,
 *                                          iterative_lsmr.jl:238.  damp MAY be clobbered (LSMR
 *                                          leaves sqrt(damp) in it, iterative_lsmr.jl:252). */
int lsq_ldiv_damped(lsq_solver *s, lsq_mat *J, const double *d_y, double *d_damp, double *d_x,
                    int *nmul);
/* LSMR(preconditioner!, P) (types.jl:82-86; README.md:47; default iterative_lsmr.jl:129-141): replace the
 * built-in Jacobi preconditioner of an LSMR solver.  Before every solve the callback must fill d_P (n
 * entries) with the factors the preconditioner solve MULTIPLIES by (an InverseDiagonal stores the
 * inverse, iterative_lsmr.jl:117-122) for the operator J'J + diag(damp); d_damp is the un-rooted
 * damping, NULL for the undamped (Dogleg) solve.  Diagonal preconditioners only.  The callback runs
 * on the host after the library's stream has been drained (the reference's slow path too); the
 * reference-order small-problem path is not used with a custom preconditioner.  NULL restores the default. */
typedef int (*lsq_precond_callback)(double *d_P, lsq_mat *J, const double *d_damp, void *user);
int lsq_solver_set_preconditioner(lsq_solver *s, lsq_precond_callback cb, void *user);
/* LSMR(preconditioner!, P) with ANY P that supports ldiv! (types.jl:82-86; README.md:47: "The preconditioner can be any type
 * that supports A_ldiv_B!(x, P, y)") -- block-diagonal, incomplete factors, whatever the caller keeps behind `user`:
 *   update(J, d_damp, user) = preconditioner!(P, x, J, damp): refresh P for J'J + diag(damp) (d_damp un-rooted; NULL for the
 *                             undamped Dogleg solve); may be NULL if P never changes;
 *   ldiv(d_out, d_in, user) = ldiv!(out, P, in) on n-vectors in device memory.
 * Both are HOST callbacks on device pointers; the library drains its stream before each call and the callback must have
 * finished its device work when it returns.  A general P cannot be folded into the fused kernels, so the solve runs as the
 * reference's own structure at the operator level (lsmr.jl:53-238 on PreconditionedMatrix(DampenedMatrix(J, sqrt(damp)), P),
 * every vector operation a launch, scalars on the host: lsq_lsmr_general.hip) -- the slow path, as a user-supplied P is in the
 * reference.  Like the reference (iterative_lsmr.jl:36-51) the adjoint applies ldiv!(., P, .) again, i.e. P is taken to be
 * symmetric.  ldiv = NULL restores the built-in path. */
typedef int (*lsq_precond_update_callback)(lsq_mat *J, const double *d_damp, void *user);
typedef int (*lsq_precond_ldiv_callback)(double *d_out, const double *d_in, void *user);
int lsq_solver_set_general_preconditioner(lsq_solver *s, lsq_precond_update_callback update, lsq_precond_ldiv_callback ldiv,
                                          void *user);
/* Row-sharded SINGLE problem: J is split by residual rows, rank p holds the m_p x n block J_p and the
 * matching slices of the m-vectors; every n-vector is replicated and every rank runs the same scalar control flow.  What
 * crosses ranks is a SUM all-reduce of a device buffer, IN PLACE, ordered on the library's stream (the hook enqueues it
 * there -- e.g. ncclAllReduce(d_buf, d_buf, count, ncclDouble, ncclSum, comm, hip_stream): RCCL over xGMI -- or makes that
 * stream wait for it; it must not need the host to wait).  Called per LSMR inner iteration with n + 1 doubles (J_p'u_p with
 * sum(u_p.^2) riding along: u is kept unnormalised, so the norm the reference needs BEFORE the adjoint product,
 * lsmr.jl:119-122, travels WITH it), and per outer iteration for colsumabs2 (n, only after g!), the gradient J'f (n) and
 * {trial ssr, predicted ssr} (2).  LevenbergMarquardt(LSMR()) only. */
typedef int (*lsq_device_allreduce_callback)(double *d_buf, int count, void *hip_stream, void *user);

/* row-sharded operator-level use (lsq_ldiv / lsq_ldiv_damped with LSMR on a row block J_p; y is the local slice, x the
 * replicated solution): installs the all-reduce hook of lsq_options.row_allreduce on this solver.  NULL removes it. */
int lsq_solver_set_row_allreduce(lsq_solver *s, lsq_device_allreduce_callback cb, void *user, long long global_rows);
/* diagnostics of the last solve: LSMR istop / iterations, QR numerical rank (LSQ_BLOCK_QR: the sum of the block ranks;
 * LSQ_BORDERED_QR: B*nb + the rank of the inner QR()) */
int lsq_solver_info(const lsq_solver *s, int *lsmr_iter, int *lsmr_istop, int *qr_rank);
/* which factorisation the last QR solve used (dense_qr.jl:37,83 always runs geqp3; this build only needs the
 * pivoted sweep when the rank decision is open):  0 none yet, 1 one-stage pivoted Householder,
 * 2 blocked unpivoted QR + pivoted sweep on R,  3 blocked unpivoted QR + full-rank certificate
 * (||R||_F ||inv(R)||_F * rcond * 16 <= 1 proves xGELSY's rank = n; no pivoting needed) */
int lsq_solver_qr_path(const lsq_solver *s, int *path);
/* how the 64-column panels of the last blocked QR were factored: 0 no blocked factorisation yet, 1 column-by-column
 * Householder steps (k_qr1_step_multi), 2 CholeskyQR2 + basis-kernel block reflector (lsq_qr_cholqr.hip; falls back to 1
 * for the whole solve when a panel is too ill-conditioned for it) */
int lsq_solver_qr_panel(const lsq_solver *s, int *kind);
/* the same for Cholesky() (dense_cholesky.jl:29-59):  0 none yet, 1 one-workgroup kernel (dpotf2 / pivoted dpstf2),
 * 2 blocked unpivoted factorisation (LM: J'J + damp),  3 blocked unpivoted factorisation + full-rank certificate
 * (Dogleg: 1 / ||inv(U)||_F^2 > 16 n eps max diag proves that cholesky!(.., Val(true)) would not stop early),
 * 4 like 2 with the whole factorisation in ONE launch (k_chol_chain: one resident workgroup per 64 x 64 upper tile
 * and one for the diagonal chain, n <= 1408; repeated as 2 if one of its bounded waits gives up) */
int lsq_solver_chol_path(const lsq_solver *s, int *path);
/* the same for LSMR(): which iteration driver ran the last solve.  0 none yet, 1 the reference-order kernel of small problems
 * (lsq_exact.hip), 2 the four-launch iteration (k_lsmr_update: any handle, custom diagonal preconditioners, row blocks),
 * 3 the three-launch iteration (k_lsmr_fused: both sliced layouts, one column window), 4 the operator-level recurrence of a
 * general preconditioner (lsq_lsmr_general.hip).  Read-only; the tests use it to know which copy of the stopping rules ran. */
int lsq_solver_lsmr_path(const lsq_solver *s, int *path);
/* diagnostics of the last block solve: which path (0 none yet, 1 batched unpivoted LM, 2 batched pivoted Dogleg, 3 batched
 * per-block pivoted QR: LSQ_BLOCK_QR, block = -1, 4 bordered Schur, LM: lsq_blockdiag_bordered_create, 5 the same by LSQ_SCHUR,
 * 6 bordered Householder elimination + inner QR(): LSQ_BORDERED_QR) and, after LSQ_ENOTPD /
 * LSQ_ERANK, the block that decided it (path 4: nblocks when the Schur factor of the shared columns failed) (else -1) */
int lsq_solver_blockdiag_path(const lsq_solver *s, int *path, int *block);
/* LSQ_BLOCK_QR: the numerical rank of every block in the last solve (h_ranks: nblocks ints; -1 before the first solve).
 * LSQ_EARG for a solver of another kind. */
int lsq_solver_blockdiag_ranks(const lsq_solver *s, int *h_ranks);
/* Parameter covariance at the point where J was evaluated, for the many-small-fits handles: how well each parameter is
 * determined, at the cost of ONE solve (one pass over the values) and without moving J to the host.  `s` is an LSQ_CHOLESKY
 * solver created on J (it owns the scratch and the info words, as for the solves): on a block-diagonal handle
 * (lsq_blockdiag_create, nb <= 64) either for_lm, on a bordered handle (lsq_blockdiag_bordered_create, nb + ng <= 64) for_lm = 1.
 * Any other solver kind or handle, a handle whose shape differs from the one the solver was allocated for, or d_cov and
 * d_stderr both NULL: LSQ_EARG with a message in lsq_last_error.  A column-scaled handle means J S, as everywhere else; no
 * damping is involved.  d_f: NULL (the unscaled inv(J'J)) or the residual at that point (m doubles, device).  d_cov: NULL
 * (only d_stderr is wanted) or the output below; d_stderr: NULL or n doubles, the square roots of the diagonal of what is
 * (or would be) written to d_cov, in the order of the parameters.
 *   Block-diagonal handle: d_cov is B*nb*nb doubles; block b at offset b*nb*nb is nb x nb, both triangles written with the
 *   same bits, and holds s_b^2 inv(J_b'J_b) with s_b^2 = sum(f_b.^2) / (mb - nb) over the block's own mb rows -- the residual
 *   variance of the B independent fits of lsq_optimize_batched -- or 1 without d_f.  mb <= nb with d_f: LSQ_EARG.  h_info: NULL
 *   or B host ints, entry b = 0 or the 1-based column of block b at which the unpivoted dpotrf of J_b'J_b meets a pivot that is
 *   not positive; such a block gets NaN in all of its cov and stderr entries, the other blocks are unaffected and the call
 *   returns LSQ_OK.  (LSQ_BLOCK_QR is the tool for rank-deficient blocks; a pseudo-inverse covariance is not offered.)
 *   Block b's result does not depend on the other blocks, on B, or on the run: same bits.
 *   Bordered handle: d_cov is B*nb*nb + ng*ng doubles: the B diagonal blocks of s^2 inv(J'J) that belong to the locals, then
 *   the ng x ng block of the shared parameters; ONE variance s^2 = sum(f.^2) / (m - n) (it is one fit), or 1 without d_f.
 *   m <= n with d_f: LSQ_EARG.  If a local block or the Schur factor is not positive definite: LSQ_ENOTPD with the stacked
 *   column exactly as lsq_ldiv_damped reports it (also in h_info[0] when h_info is given, else h_info[0] = 0), the block in
 *   lsq_solver_blockdiag_path, and d_cov / d_stderr unspecified.  The local-shared cross-covariances -W_b Cov_gg
 *   (W_b = inv(J_b'J_b) J_b'C_b) are NOT formed.
 * Synchronises the stream when it has host results to return (h_info, the bordered handle's status); otherwise stream-ordered. */
int lsq_solver_covariance(lsq_solver *s, lsq_mat *J, const double *d_f, double *d_cov, double *d_stderr, int *h_info);
/* The same for the plain dense J::Matrix of the reference (lsq_dense_create; the handle of LevenbergMarquardt(Cholesky()),
 * dense_cholesky.jl:43-59, Dogleg(Cholesky()), :29-35, and QR(), dense_qr.jl:30-88): Cov = s^2 inv(J'J) without moving J to
 * the host.  lsq_solver_covariance keeps refusing dense handles; this is the entry point beside it.  `s` is an LSQ_CHOLESKY
 * solver created on J, either for_lm (it owns the scratch: the first call allocates 2 n^2 doubles for inv(U) and its
 * workspace).  A solver of another kind, a handle that is not dense (CSC, block-diagonal, bordered, operator), a shape that
 * differs from the solver's, or d_cov and d_stderr both NULL: LSQ_EARG with a message in lsq_last_error.  A column-scaled
 * dense handle means J S.  No damping is involved; J and d_f are not written.
 *   d_f: NULL (the unscaled inv(J'J)) or the residual (m doubles, device): s^2 = sum(f.^2) / (m - n) through lsq_sumsq, as
 *   for the bordered handle.  m <= n with d_f: LSQ_EARG.
 *   d_cov: NULL or n*n doubles, column-major, both triangles written with the same bits.
 *   d_stderr: NULL or n doubles, s * sqrt(sum_{k >= i} X_ik^2) with X = inv(U), J'J = U'U.  They come from a kernel of their
 *   own with a fixed summation order: the same bits whether or not d_cov is asked for.  They agree with sqrt(diag(cov)) to
 *   rounding, NOT bit for bit (the covariance adds the same squares in the matrix unit's order).
 * J'J = U'U is the unpivoted factorisation of the damped solve with no damping added.  A pivot that is not positive:
 * LSQ_ENOTPD, the 1-based column at which the unpivoted dpotrf of J'J stops in the message -- the one lsq_ldiv_damped sets --
 * and in h_info[0] when h_info is given (0 on success); d_cov / d_stderr are then unspecified, and the solver remains usable
 * for solves and for further covariances.  (A pseudo-inverse for rank-deficient J is not offered.  The covariance from
 * the QR() factor, which does not square the condition number, is lsq_dense_qr_covariance below.)
 * The result has the same bits on every run, under lsq_debug_set(serial = 1), and for either for_lm.  lsq_solver_chol_path
 * afterwards reports the factorisation that was used: 2 or 4 (1 for the few operands that lsq_ldiv_damped, too, keeps in one
 * workgroup: n < 32 with m * n < 20000, or n = 1).  Waits for the stream once, in the middle -- for the info word and s^2,
 * which are read back to back; the last two launches are stream-ordered behind that. */
int lsq_dense_covariance(lsq_solver *s, lsq_mat *J, const double *d_f, double *d_cov, double *d_stderr, int *h_info);
/* The same from the QR() factor (dense_qr.jl:30-88): Cov = s^2 inv(J'J) = s^2 P X X' P' with J P = Q R, X = inv(R).  J'J is
 * never formed, so the condition number is not squared: the result keeps its digits where lsq_dense_covariance has lost them
 * (cond(J) towards 1e8) or returns LSQ_ENOTPD.  `s` is an LSQ_QR solver created on the dense handle J (lsq_dense_create),
 * either for_lm.  A column-scaled handle means J S.  No damping is involved; J and d_f are not written.
 * LSQ_EARG, each with a message in lsq_last_error: a solver of another kind; a handle that is not dense; a shape that differs
 * from the solver's; m < n; d_cov and d_stderr both NULL; d_f with m <= n.
 *   d_f: NULL (s^2 = 1) or the residual (m doubles, device): s^2 = sum(f.^2) / (m - n) through lsq_sumsq.
 *   d_cov: NULL or n*n doubles, column-major, in parameter order; both triangles are written with the same bits.
 *   d_stderr: NULL or n doubles in parameter order, from a kernel of their own with a fixed summation order: the same bits
 *   with and without d_cov.  They agree with sqrt(diag(cov)) to rounding only.
 * The factor is whatever lsq_ldiv enqueues for this operand -- the one-workgroup kernel, the multi-CU pivoted Householder, the
 * two-stage factorisation with CholeskyQR2 or Householder panels, TSQR levels, the full-rank certificate or the pivoted sweep
 * on R, and the retries after an exchange gives up or a CholeskyQR2 panel breaks down -- run on a solver-owned zero
 * right-hand side whose solution is discarded; a for_lm solver stacks n zero rows under J (the same R, and the workspace of its
 * solves stays).  On the certified path X is the inverse the certificate has formed; elsewhere the pivoted triangle is
 * inverted (the first such call allocates 2 n^2 doubles) and the result is un-permuted on the way out.
 * The rank is the decision of the solves: xGELSY's at rcond = n eps (lsq_solver_info's qr_rank), or n when the certificate
 * holds.  h_info[0] (when given) receives it.  rank < n: LSQ_ERANK with a message that states rank and n; d_cov / d_stderr are
 * then unspecified and the solver stays usable for solves and further covariances.  A pseudo-inverse is not offered.
 * lsq_solver_qr_path / lsq_solver_qr_panel afterwards report the factorisation that ran.  The result has the same bits on
 * every run and under lsq_debug_set(serial = 1); for_lm = 0 and for_lm = 1 solvers agree to rounding only (the stacked operand
 * is split into other slabs).  Waits where the solve waits (the certificate's copy) and once more, for the rank and s^2, which
 * are read back to back; the last two launches are stream-ordered behind that. */
int lsq_dense_qr_covariance(lsq_solver *s, lsq_mat *J, const double *d_f, double *d_cov, double *d_stderr, int *h_info);
/* The same for a bordered block-diagonal Jacobian J = [blkdiag(J_1 .. J_B) | C] (lsq_blockdiag_bordered_create), from the
 * factor of LSQ_BORDERED_QR, with the local-shared cross-covariances: Cov = s^2 inv(J'J) with ONE variance
 * s^2 = sum(f.^2) / (m - n), m = B*mb, n = B*nb + ng.  Neither J'J nor any part of it is formed, so the condition number is not
 * squared.  `s` is an LSQ_BORDERED_QR solver created on the handle J (nb <= 64, any ng >= 1, for_lm = 1).  A column-scaled
 * handle means J S.  No damping is involved; J and d_f are not written.
 *   d_f: NULL (s^2 = 1) or the residual (m doubles, device), summed through lsq_sumsq.
 *   d_cov: NULL or B*nb*nb + ng*ng doubles in lsq_solver_covariance's layout for this handle: the B local blocks, then the
 *   shared block; every block is written with both triangles holding the same bits.
 *   d_stderr: NULL or n doubles in parameter order: the same bits whichever of d_cov / d_cross is asked for as well.  They agree
 *   with sqrt(diag(cov)) to rounding only.
 *   d_cross: NULL or (B*nb) x ng doubles, column-major with leading dimension B*nb: row b*nb + i, column j is
 *   Cov(local i of block b, shared j) -- the off-diagonal panel of the full covariance matrix in parameter order.
 *   h_info: NULL or 2 ints.  h_info[0]: 0, or the 1-based stacked column b*nb + k at which some R_b has a zero or non-finite
 *   diagonal entry (the lowest wins: the column lsq_ldiv_damped names); h_info[1]: the rank the inner QR() decided.
 * With zero damping the elimination of LSQ_BORDERED_QR leaves per block Q_b'[J_b C_b] = [R_b W_b; 0 F_b].  Cgg = inv(F'F) is
 * lsq_dense_qr_covariance on the solver's own inner QR() (every factorisation path and retry it has; an ng x ng buffer owned
 * by the solver, allocated at the first call with m zeros for the elimination's damping and right-hand side); then
 * T_b = inv(R_b) W_b in place of W, the tall product P = T Cgg ((B*nb) x ng times ng x ng, on the fp64 matrix unit), and per
 * block Cov_bb = s^2 (inv(R_b) inv(R_b)' + P_b T_b'); Cov_gg = s^2 Cgg, Cov_bg = -s^2 P_b.  P stands in the solver's own
 * workspace (the place of F): no output-sized buffer is allocated that the caller did not ask for.
 * A failing local column: LSQ_ERANK with LSQ_BORDERED_QR's message and column.  An inner rank < ng: LSQ_ERANK with a message
 * that states rank and ng.  The outputs are then unspecified; the solver stays usable for solves and further covariances, and
 * a solve after a covariance has the bits of a solve without one.  A pseudo-inverse is not offered.
 * LSQ_EARG, each with a message that names the alternative: a solver of another kind; a handle that is not bordered; a shape
 * other than the solver's; m < n; d_f with m <= n; d_cov, d_stderr and d_cross all NULL.
 * Waits where the inner QR() waits and once more, for the locals' verdict, the rank and s^2, which are read back to back; the
 * launches after that are stream-ordered.  No floating-point atomics, no workgroup waits for another, every sum has a fixed
 * association: the same bits on every run, on a second solver and under lsq_debug_set(serial = 1). */
int lsq_bordered_qr_covariance(lsq_solver *s, lsq_mat *J, const double *d_f, double *d_cov, double *d_stderr, double *d_cross,
                               int *h_info);
/* G = J'J (+ diag(d_damp)) of a sparse Jacobian as a dense matrix, formed on the device without densifying J (k_sp_gram,
 * lsq_cov_sparse.hip).  J: any LSQ_MAT_CSC handle -- lsq_csc_create, lsq_blockdiag_create, lsq_blockdiag_bordered_create -- at
 * the values it holds; a column-scaled handle means J S.  d_damp: NULL or n doubles added to the diagonal.  d_G: n x n doubles,
 * column-major: the upper triangle and the diagonal are written, the strict lower triangle is left alone.  Enqueues one kernel;
 * stream-ordered, nothing is returned to the host.  Every entry is a sum over the rows that columns k and j share, taken in
 * the order of column j's stored entries by one wavefront: no floating-point atomics, the same bits on every run and under
 * lsq_debug_set; two columns that share no row give an exact 0.
 * LSQ_EARG, each with a message in lsq_last_error: a dense handle, an operator handle, n > 16384 (one accumulator column of n
 * doubles must fit the LDS of a workgroup).  n = 0: LSQ_OK, nothing is launched. */
int lsq_sparse_gram(lsq_mat *J, const double *d_damp, double *d_G);
/* lsq_dense_covariance, argument for argument, for a general sparse Jacobian: Cov = s^2 inv(J'J) without moving J to the host.
 * J: an LSQ_MAT_CSC handle (plain, block-diagonal or bordered; for the latter two lsq_solver_covariance works block by block
 * and has no limit on n); `s`: the LSQ_LSMR solver created on it, the one a sparse fit already owns.  The first call gives that
 * solver an inner dense Cholesky() solver (n^2 doubles for J'J, 2 n^2 more for inv(U) and its workspace), freed with it.
 *   d_f: NULL (the unscaled inv(J'J)) or the residual (m doubles, device): s^2 = sum(f.^2) / (m - n) through lsq_sumsq.
 *   d_cov: NULL or n*n doubles, column-major, both triangles written with the same bits.  NULL allocates and writes no n x n
 *   output: the standard errors alone are n doubles.
 *   d_stderr: NULL or n doubles, from a kernel of their own with a fixed summation order: the same bits with and without d_cov.
 * Launches, in stream order: lsq_sparse_gram's kernel into the inner solver, the factorisation of the dense damped solve with
 * no damping added (one launch, or a launch per panel; the one-workgroup kernel where lsq_dense_covariance uses it), the
 * explicit inverse of the factor, and the last two kernels of lsq_dense_covariance.  Waits for the stream once, in the middle,
 * for the info word and s^2.  If the one-launch factorisation gives up on a wait, the Gram kernel and the panel launches run
 * once more (lsq_solver_stats of `s`, index 0, counts it).  lsq_solver_chol_path of `s` afterwards reports 1, 2 or 4.
 * A pivot that is not positive -- a structurally empty column among them: LSQ_ENOTPD, the 1-based column in the message and
 * in h_info[0] when given (0 on success); the solver stays usable.  The result has the same bits on every run and under
 * lsq_debug_set(serial = 1).
 * LSQ_EARG, each with a message that names the alternative: a dense handle (lsq_dense_covariance), an operator handle, a
 * solver that is not LSMR() or was created for another shape, a solver with a row all-reduce hook, d_cov and d_stderr both
 * NULL, d_f with m <= n, n > 16384.  n = 0: LSQ_OK, nothing is launched. */
int lsq_sparse_covariance(lsq_solver *s, lsq_mat *J, const double *d_f, double *d_cov, double *d_stderr, int *h_info);
/* Leverages and prediction variances of a dense fit from the QR() factor: the quadratic form q(a) = a' inv(J'J) a = ||X' P' a||^2
 * with J P = Q R, X = inv(R), for the rows of J itself (q_i = h_i, the diagonal of the hat matrix J inv(J'J) J') or for new
 * rows, and what follows from it and the residual.  J'J is never formed, and neither the n x n covariance nor J leaves the
 * device.  `s` is an LSQ_QR solver created on the dense handle J (lsq_dense_create), either for_lm.  The factor, the rank
 * decision, the retries and the allocation rules are those of lsq_dense_qr_covariance (above): whatever lsq_ldiv enqueues for
 * this operand, run on a solver-owned zero right-hand side.  No damping is involved; J, d_A and d_f are not written; a solve
 * after this call has the bits of a solve without it.
 *   d_A = NULL: the rows of J; p and lda are ignored, there are m outputs and q_i = h_i.  A column-scaled handle means J S, as
 *   everywhere else.
 *   d_A non-NULL: p >= 1 rows in the parameter space the handle means (for a column-scaled handle: of J S), column-major as
 *   p x n with leading dimension lda >= p (device); there are p outputs.  d_student and d_cook must then be NULL.
 *   d_f: NULL, or the residual (m doubles, device).  d_se, d_student, d_cook and h_s2 need it.
 *   d_q: NULL or the quadratic forms.  d_se, d_student, d_cook: NULL or, with s2 = lsq_sumsq(f) / (m - n) (also written to
 *   *h_s2, a host double, when that is given), each line one IEEE operation in exactly this order:
 *       sd     = sqrt(s2)
 *       se_i   = sd * sqrt(q_i)                         the standard error of the prediction a_i'x: the band is y^ +- t * se
 *       d_i    = 1 - h_i
 *       t_i    = f_i / (sd * sqrt(d_i))                 the internally studentized residual
 *       cook_i = ((t_i * t_i) * h_i) / (n * d_i)        Cook's distance, n converted to double
 *   Nothing is clamped: an h_i that rounds to 1 or above (a row that alone determines a parameter) gives what IEEE arithmetic
 *   gives for these lines -- a division by zero, the square root of a negative number: +-inf or NaN in t_i and cook_i.
 *   h_info: NULL or one int, the rank the solve decided.
 * The hot path is one kernel on the fp64 matrix unit (k_lev_tall, lsq_leverage.hip): one workgroup per 64 rows, Z = A P X
 * accumulated tile by tile with k in index order and squared into the row sums at once; Z is never stored.  Row i's bits
 * depend on row i and on X only: not on p, on where the row stands, on the other rows, on the run, or on
 * lsq_debug_set(serial = 1); d_A = the values of J gives the bits of d_A = NULL.  No floating-point atomics.  When d_q is NULL
 * and a derived output is asked for, the solver keeps the q's in a buffer of its own (grown on demand, freed with it).
 * rank < n: LSQ_ERANK with lsq_dense_qr_covariance's message (rank and n); the outputs are unspecified and the solver stays
 * usable for solves, covariances and further leverages.  A pseudo-inverse is not offered.
 * LSQ_EARG, each with a message in lsq_last_error: a solver of another kind; a handle that is not dense; a shape other than the
 * solver's; m < n; every output NULL; d_f with m <= n; d_se, d_student, d_cook or h_s2 without d_f; d_student or d_cook with
 * d_A; p < 1 or lda < p with d_A.
 * Waits where lsq_dense_qr_covariance waits; the launches behind the rank are stream-ordered. */
int lsq_dense_qr_leverage(lsq_solver *s, lsq_mat *J, const double *d_A, int p, int lda, const double *d_f, double *d_q,
                          double *d_se, double *d_student, double *d_cook, double *h_s2, int *h_info);
/* The same for a block-diagonal Jacobian (lsq_blockdiag_create, nb <= 64): B independent fits, one per block, in one pass --
 * the handle and the limits of lsq_solver_covariance.  `s` is an LSQ_CHOLESKY solver created on J, either for_lm.  A
 * column-scaled handle means J S.  Outputs (device; any may be NULL, not all): d_h, d_se, d_student, d_cook: m = B*mb doubles
 * in row order; d_s2: B doubles, s_b^2 = sum(f_b.^2) / (mb - nb) over the block's own rows, summed in lsq_solver_covariance's
 * fixed order.  The lines above hold per block with s2 = s_b^2 and n = nb.  d_f: NULL (then only d_h may be asked for) or the
 * residual.  The factor is a CholeskyQR2: J_b'J_b = U_b'U_b, the unpivoted factorisation of lsq_solver_covariance, then
 * z_i = inv(U_b)' a_i, sum z z' = U2'U2 and h_i = ||inv(U2)' z_i||^2 -- three passes over the values, every sum in index order --
 * so that the leverages keep the accuracy of a QR (cond(J_b) u, not cond(J_b)^2 u) wherever the first factorisation succeeds.
 * h_info: NULL or B host ints, entry b = 0 or the 1-based column at which block b's factorisation
 * meets a pivot that is not positive: such a block gets NaN in all of its mb rows of every output and in d_s2[b], the other
 * blocks are unaffected and the call returns LSQ_OK.  Block b's bits do not depend on B, on the other blocks or on the run.
 * LSQ_EARG with a message that names the alternative: a bordered, dense, CSC or operator handle; a solver of another kind or
 * shape; every output NULL; d_f with mb <= nb; d_se, d_student, d_cook or d_s2 without d_f.
 * Stream-ordered; synchronises only to return h_info.  New rows on this handle are not offered. */
int lsq_solver_leverage(lsq_solver *s, lsq_mat *J, const double *d_f, double *d_h, double *d_se, double *d_student,
                        double *d_cook, double *d_s2, int *h_info);
/* lsq_dense_qr_leverage for a bordered block-diagonal Jacobian J = [blkdiag(J_1 .. J_B) | C] (lsq_blockdiag_bordered_create), the
 * Jacobian of a global fit, from the factor of LSQ_BORDERED_QR: which points of which data set drive the shared parameters, and
 * the confidence band of curve b.  `s` is an LSQ_BORDERED_QR solver created on J (nb <= 64, any ng >= 1, for_lm = 1).  Neither
 * J'J nor the n x n covariance is formed, so the condition number is not squared.  A column-scaled handle means J S.  No damping
 * is involved; J, the new rows and d_f are not written.
 *   d_Ab = d_Ag = NULL: the m = B*mb rows of J in row order, q_i = h_i; block, p, ldab and ldag are ignored.
 *   d_Ab and d_Ag both non-NULL: p >= 1 new rows of block `block` (0 <= block < B) in the parameter space the handle means:
 *   d_Ab their local parts, p x nb column-major with leading dimension ldab >= p, d_Ag their shared parts, p x ng with leading
 *   dimension ldag >= p (device); there are p outputs.  d_student and d_cook must then be NULL.
 *   d_f, d_q, d_se, d_student, d_cook, h_s2: as for lsq_dense_qr_leverage, line for line, with ONE variance
 *   s2 = lsq_sumsq(f) / (m - n), m = B*mb, n = B*nb + ng, and that n in Cook's distance.
 *   h_info: NULL or 2 ints, as for lsq_bordered_qr_covariance: h_info[0] 0 or the 1-based stacked column of a failing local,
 *   h_info[1] the rank the inner QR() decided.
 * With zero damping the elimination of LSQ_BORDERED_QR leaves per block Q_b'[J_b C_b] = [R_b W_b; 0 F_b], and F P = Q_g R_g is
 * the solver's inner QR() (X_g = inv(R_g) as lsq_dense_qr_covariance forms it; the zeros of the elimination stand in the buffer
 * lsq_bordered_qr_covariance allocates at its first call).  For a row with local part a_b and shared part c:
 *       z = inv(R_b)' a_b      e = c - W_b' z      u = inv(R_g)' P' e      q = ||z||^2 + ||u||^2
 * k_bl_local (lsq_lev_bordered.hip): one workgroup per (block, 64 rows), R_b and Z in LDS, a forward substitution per row,
 * ||z||^2 summed in index order, E = C - Z W_b on the fp64 matrix unit with k in index order; for J's own rows E stands in the
 * solver's workspace (the place of F, of which the inner QR() has its copy), for new rows in a solver-owned buffer grown on
 * demand.  Then lsq_dense_qr_leverage's kernel on E with X_g and the inner pivots, one IEEE addition q = ||z||^2 + ||u||^2, and
 * the derived lines above.  Row i's bits depend on row i and on the factor only: not on p, on where the row stands, on the
 * other rows, on which outputs are asked for, on the run, or on lsq_debug_set(serial = 1); on a handle without a column scale
 * a block's own rows passed as new rows give the bits of d_Ab = NULL.  No floating-point atomics.
 * A failing local column or an inner rank < ng: LSQ_ERANK with lsq_bordered_qr_covariance's messages and h_info.  The outputs
 * are then unspecified; the solver stays usable for solves, covariances and leverages, and a solve or a covariance after a
 * leverage has the bits of one without it.
 * LSQ_EARG, each with a message that names the alternative: a solver of another kind; a handle that is not bordered; a shape
 * other than the solver's; m < n; every output NULL; d_f with m <= n; d_se, d_student, d_cook or h_s2 without d_f; d_student or
 * d_cook with new rows; only one of d_Ab and d_Ag; block out of range; p < 1 or a leading dimension below p.
 * Waits where lsq_bordered_qr_covariance waits; the launches behind that are stream-ordered. */
int lsq_bordered_qr_leverage(lsq_solver *s, lsq_mat *J, int block, const double *d_Ab, int ldab, const double *d_Ag, int ldag,
                             int p, const double *d_f, double *d_q, double *d_se, double *d_student, double *d_cook,
                             double *h_s2, int *h_info);

/* The fast paths above that rely on co-resident workgroups (one-launch Cholesky, pipelined triangular solves, the QR panel's slab
 * exchange + pipelined certified solve) wait with a bound; a wait that gives up makes the solve repeat itself on the
 * launch-per-step path, is COUNTED, and pauses that fast path for a number of solves (16, then 64, ... up to 4096 while it
 * keeps failing right after being armed again; back to 16 after a clean run) instead of switching it off for good: a
 * neighbour on the device (an RCCL kernel of a sharded run) may be gone by then.  Index: 0 one-launch Cholesky (k_chol_chain),
 * 1 pipelined triangular solves, 2 QR slab exchange / pipelined certified solve, 3 CholeskyQR2 panel breakdowns (numerical:
 * ill-conditioned panels -- counted and paused the same way).  h_giveups: totals of this solver; h_paused: solves left before
 * the path is tried again (0 = armed).  Either pointer may be NULL. */
int lsq_solver_stats(const lsq_solver *s, int h_giveups[4], int h_paused[4]);
/* the same totals over every solver the context has run (the solver lsq_optimize keeps inside the context included) */
int lsq_ctx_fallback_stats(const lsq_ctx *ctx, int h_giveups[4]);
/* What the context's device looks like to the launch heuristics: compute units (256 on an unpartitioned MI355X, 32 in CPX mode:
 * the slab exchanges of the QR panel need all 256 -- lsq_qr_stage1.hip), XCDs inferred from that (8 CUs x 4 per XCD -> num_cus / 32),
 * and the architecture name (at most name_cap - 1 characters).  Any pointer may be null. */
int lsq_ctx_device_info(const lsq_ctx *ctx, int *num_cus, int *num_xcds, char *arch_name, int name_cap);

/* LM + LSMR with a device-side f!: the kernels that follow the inner solve (step, predicted residual, trial residual) are
 * enqueued behind the inner iteration at which the PREVIOUS solve stopped and skip themselves if this one is not over by then
 * (DESIGN 4.2).  h_out = {solves that were given such a guess, guesses that were wrong}; LSQ_NO_TAIL_SPECULATION=1 turns it off. */
int lsq_ctx_tail_stats(const lsq_ctx *ctx, long long h_out[2]);
/* Where the three-launch LSMR iteration expects the stop and its caller is the LM loop, one narrow launch (k_lsmr_commit_step)
 * decides the iteration and, if the solve is over, takes the trust-region step as well.  h_out = {such launches that found the
 * solve over, such launches that found it unfinished}; LSQ_NO_COMMIT_STEP=1 turns them off (cautious launches and k_step). */
int lsq_ctx_commit_step_stats(const lsq_ctx *ctx, long long h_out[2]);

/* ---- whole trust-region loop on device buffers (host control, device arrays) ---- */
/* f!(out, x) and g!(J, x) on DEVICE pointers; g writes lsq_mat_values(J) (the library refreshes
 * the CSR mirror afterwards).  Return non-zero to abort with LSQ_ECALLBACK. */
typedef int (*lsq_f_callback)(double *d_out, const double *d_x, void *user);
typedef int (*lsq_g_callback)(lsq_mat *J, const double *d_x, void *user);
/* optional global reduction hook for sharded problems: called exactly once per outer
 * iteration with vals = {ssr_local, maxabs_gr_local, converged_local} (the values the rank held at
 * the top of the iteration); it overwrites them with the global {sum, max, min}.  NULL = single
 * problem.  A rank that reports converged_local = 1 is frozen: it is called at the top of the
 * iteration and leaves the loop when the returned min is 1.  A rank that is still iterating is
 * called LATER in the iteration, once device work has been queued (inside the LSMR driver when its
 * look-ahead window is full), so the exchange overlaps the device; it never acts on the result
 * ("all converged" cannot hold while it is not converged itself), which lets an implementation
 * return the previous exchange's values to such a rank and leave the new one in flight
 * (leastsquaresoptim.jl_amd/sharding.py does; bench.py carries it over the RCCL process group).
 * Error protocol: a rank that leaves its loop with an error calls the hook one last time with
 * converged_local = -1; an implementation reports "some rank has left" to the others either by returning 2
 * or by setting the returned third value to -1 -- the loop then returns LSQ_ERCCL instead of entering another
 * collective that the departed rank will never join. */
typedef int (*lsq_allreduce_callback)(double *h_vals, int count, void *user);

typedef struct {
    double x_tol, f_tol, g_tol; /* 1e-8 defaults of levenberg_marquardt.jl:41 / dogleg.jl:43 */
    int iterations;             /* 1000 */
    double delta;               /* <= 0: 10.0 for LM, 1.0 for Dogleg */
    const double *h_lower;      /* NULL or n (host) */
    const double *h_upper;      /* NULL or n (host) */
    lsq_allreduce_callback allreduce;
    void *allreduce_user;
    /* optional trace buffers (host), capacity trace_cap iterations */
    int trace_cap;
    double *trace_ssr, *trace_gnorm, *trace_delta, *trace_rho;
    int *trace_inner, *trace_accept;
    double *trace_x;            /* trace_cap * n, or NULL */
    lsq_precond_callback preconditioner;   /* LSMR only; NULL = default Jacobi */
    void *preconditioner_user;
    lsq_device_allreduce_callback row_allreduce;   /* row-sharded single problem (see above); NULL = J holds all rows */
    void *row_allreduce_user;
    long long global_rows;      /* row-sharded: sum of the ranks' row counts (lsmr.jl:55 maxiter = max(size(A)...)) */
    lsq_precond_update_callback precond_update;    /* LSMR(preconditioner!, P) with a general P (see */
    lsq_precond_ldiv_callback precond_ldiv;        /* lsq_solver_set_general_preconditioner); NULL = not used */
    void *precond_general_user;
} lsq_options;

typedef struct {
    int optimizer;              /* lsq_optimizer_kind actually used */
    double ssr;
    int iterations;
    int converged, x_converged, f_converged, g_converged;
    int f_calls, g_calls, mul_calls;
    int status;
    int bad_index;              /* for LSQ_ENONFINITE */
    double seconds;             /* wall time of the loop (host clock, includes syncs) */
    long long lsmr_iterations;  /* total inner iterations */
    double ssr0;                /* sum(abs2, f(x0)): state 0 of the reference's trace (levenberg_marquardt.jl:70) */
} lsq_result;

void lsq_options_default(lsq_options *opt);
/* optimize!(LeastSquaresProblemAllocated; kwargs...) -- levenberg_marquardt.jl:39-144,
 * dogleg.jl:41-203.  d_x (n) and d_fcur (m) are updated in place like nls.x / nls.y.
 * g = NULL is the reference's default problem (types.jl:54-58): wherever the loop would call g! it takes the central-difference
 * Jacobian of f on the device (lsq_fd_jacobian below, same handles, same bits).  f_calls counts the optimizer's own evaluations
 * only (the reference's closure calls f! inside g! uncounted), g_calls as with a callback.  A handle lsq_fd_jacobian refuses:
 * LSQ_EARG with the reason in lsq_last_error.  lsq_optimize_batched takes g = NULL the same way. */
int lsq_optimize(lsq_ctx *ctx, int optimizer, int solver_kind, lsq_mat *J, double *d_x,
                 double *d_fcur, lsq_f_callback f, lsq_g_callback g, void *user,
                 const lsq_options *opt, lsq_result *res);
/* The Jacobian of f at d_x by central differences, on the device, written into lsq_mat_values(J) and followed by what the
 * loops do after a g! callback (lsq_mat_refresh: every layout of the handle sees the new values).  This is the g! of the
 * reference's default problem, LeastSquaresProblem(x, y, f!) without g! (types.jl:54-58).  d_x: n doubles, not written.
 * The step of entry j is h = max(eps3 |x_j|, eps3) with eps3 = 0x1.965fea53d6e41p-18; x_j + h and x_j - h are formed from
 * x_j, the column is (f(x+) - f(x-)) / (2 h), each operation correctly rounded: the bits a host loop in IEEE doubles gives.
 * Columns that no residual row shares are perturbed in ONE pair of evaluations (a colour), and f always sees full vectors:
 *   dense m x n (lsq_dense_create): n colours, one column each;
 *   block-diagonal (lsq_blockdiag_create): nb colours -- colour c is column c of EVERY block, each with its own h -- so a
 *     Jacobian costs 2 nb evaluations of f whatever the number of blocks is; f must be block-separable, as the handle says;
 *   bordered (lsq_blockdiag_bordered_create): those nb colours, then one per shared column: 2 (nb + ng) evaluations;
 *   plain CSC (lsq_csc_create): the colouring attached with lsq_mat_set_fd_colouring below, 2 ncolours evaluations.
 * f is called as f(d_fplus, d_xplus, user), then f(d_fminus, d_xminus, user), colour by colour in that order; besides them
 * the stream carries one launch per colour and one in front.  The scratch (two work copies of x, f+ and f-) belongs to the
 * handle: allocated by the first call, freed by lsq_mat_destroy.  Stream-ordered; no host wait of its own.
 * A non-zero return of f: LSQ_ECALLBACK (the handle stays usable; its values are then a mix of old and new columns).
 * LSQ_EARG, with the reason in lsq_last_error: a plain CSC handle without a colouring (a general sparse pattern needs a column
 * colouring: lsq_mat_set_fd_colouring), an operator handle, a handle with a column scale set (lsq_mat_set_colscale), a null
 * argument. */
int lsq_fd_jacobian(lsq_ctx *ctx, lsq_mat *J, const double *d_x, lsq_f_callback f, void *user);

/* ---- central differences on a general sparse pattern: column colourings ----
 * A colouring gives every column a colour 0 .. ncolours-1 so that the columns of one colour can be perturbed in one pair of
 * evaluations of f.  It is VALID when no row of the pattern holds two columns of one colour; the largest number of entries in
 * a row is therefore a lower bound on the number of colours of any valid colouring.
 * lsq_csc_greedy_colouring (host arrays only, no context): first fit in natural column order -- colour[j] is the smallest
 * c >= 0 that no column k < j sharing a row with j holds, an empty column gets 0.  Deterministic; sum over the rows of
 * (entries of the row)^2 steps, O(n + nnz) memory.  h_colour: n ints, h_ncolours: one.  The pattern errors of lsq_csc_create
 * (LSQ_EDIM / LSQ_EARG). */
int lsq_csc_greedy_colouring(int m, int n, const int *h_colptr, const int *h_rowval, int *h_colour, int *h_ncolours);
/* Attach a colouring to a plain CSC handle (lsq_csc_create): from then on lsq_fd_jacobian and g = NULL in lsq_optimize take
 * it (every solver the handle takes).  h_colour_or_null: n host ints, NULL = the greedy colouring of the handle's own pattern;
 * *h_ncolours (may be NULL) receives the number of colours.  A given array is checked in O(nnz + n): every value >= 0, every
 * value 0 .. max used at least once, no row with two columns of one colour (the message names the row and the two columns);
 * else LSQ_EARG and the handle keeps what it had.  Dense, block-diagonal and bordered handles have their built-in colouring
 * and an operator has no values: LSQ_EARG with the reason.  A second call replaces the first; the tables (O(n) on the host
 * and on the device) belong to the handle and go with lsq_mat_destroy; uploads of values, lsq_mat_refresh and
 * lsq_mat_set_colscale leave them alone (a column scale is refused by lsq_fd_jacobian as on any handle).
 * THE CONTRACT: the pattern must contain every (row, column) on which f depends.  A dependence that has no entry is not
 * detected: it silently corrupts the other columns of that colour in that row.  An entry f does not depend on receives 0.
 * The stream per Jacobian is as above: one launch in front, then per colour f, f and one launch, which writes every stored
 * entry of the colour exactly once (balanced by stored entries, not by columns); about 28 bytes per stored entry in all. */
int lsq_mat_set_fd_colouring(lsq_mat *J, const int *h_colour_or_null, int *h_ncolours);
/* The attached colouring: *h_ncolours = 0 when none is attached; h_colour (n ints, may be NULL) is written otherwise. */
int lsq_mat_fd_colouring(const lsq_mat *J, int *h_colour, int *h_ncolours);

/* ---- B independent fits stacked on a block-diagonal Jacobian: one trust region PER BLOCK ----
 * For every block b of J = blkdiag(J_1 .. J_B) (lsq_blockdiag_create, nb <= 64) this runs the reference's optimize!
 * (levenberg_marquardt.jl:39-144 / dogleg.jl:41-203 with Cholesky(), dense_cholesky.jl:29-59) on the mb x nb problem made of
 * residual rows b*mb .. (b+1)*mb-1 and parameters b*nb .. (b+1)*nb-1: its own delta (10 / 1; Dogleg: times wnorm(x_b, dtd_b)
 * at its first iteration, dogleg.jl:92-97), decrease_factor (levenberg_marquardt.jl:53,136-137) or reuse flag with the cached
 * Gauss-Newton / gradient steps (dogleg.jl:59-62,81), its own mean of dtd over ITS nb columns (levenberg_marquardt.jl:84-85),
 * rho, accept / revert, assess_convergence (utils.jl:7-31) and iteration count; f_calls / g_calls / mul_calls are what that
 * block's own run of the reference would count.  A block that has converged, reached opt->iterations or failed is frozen: its
 * x_b, fcur_b, ssr and counters never change again and no solve work is done for it; the call returns when no block is active.
 * x_tol, f_tol, g_tol, iterations, delta apply to every block; h_lower / h_upper are NULL or of length n.
 * A failure of ONE block does not end the call: its status[b] becomes LSQ_ENOTPD (LM; info[b] = the 1-based column of the
 * block at which dpotrf stops), LSQ_ERANK (Dogleg; info[b] = the rank of the block's pivoted factorisation) or LSQ_ENONFINITE
 * (check_isfinite, utils.jl:70-75; info[b] = the first non-finite index inside the block), it keeps the iterate it held and
 * the others go on; the call returns LSQ_OK.  Callback failures, HIP errors and bad arguments are call-level.
 * With LSQ_BLOCK_QR the per-block solver is the reference's QR() (dense_qr.jl:30-88) instead: a block never fails on rank,
 * status[b] stays LSQ_OK and info[b] is the numerical rank of the block's last solve (-1 only where nothing was solved) --
 * under LevenbergMarquardt that is the rank of [J_b; diag(sqrt(damp_b))], nb for any positive damping, under Dogleg of J_b;
 * LSQ_ENONFINITE is as above.
 * f and g are the callbacks of lsq_optimize on the stacked x (n), residual (m) and lsq_mat_values(J); they must be
 * block-separable (rows of block b depend on x_b only -- what a block-diagonal Jacobian says) and deterministic.  They are
 * called once per outer iteration for all blocks: g is handed, for every block that does not need a new Jacobian, the x_b at
 * which that block's Jacobian was last evaluated (the reference does not re-evaluate J_b at a reverted iterate,
 * levenberg_marquardt.jl:135), and the trial point holds a frozen block's final x_b; what f writes into the rows of frozen
 * blocks is ignored.  g = NULL: central differences of f (lsq_fd_jacobian) at those same per-block points, every block rewritten --
 * a block that did not want its Jacobian gets the bits it already holds; its 2 nb evaluations of f are not counted in f_calls.
 * Refused with LSQ_EARG: a handle that is not block-diagonal, nb > 64, LSQ_QR, LSQ_LSMR, and any of
 * allreduce / row_allreduce / the preconditioner hooks in the options.
 * All arrays of the result are HOST arrays owned by the caller, of length B unless said otherwise; any may be NULL.  The
 * trace (trace_cap > 0 and all six trace pointers set): row k, 0-based, of block b -- [k * B + b], x: [k * n + b * nb ..] --
 * is that block's state after its iteration k + 1 and only meaningful for k < iterations[b].
 * `batched_result` points to an lsq_batched_result (spelled void * here: the header lint of tests/julia_shim_lint.py classifies
 * parameter types from a closed list). */
typedef struct {
    double *ssr, *ssr0;         /* sum(abs2, fcur_b) at the end / at x0 */
    int *iterations;
    int *converged, *x_converged, *f_converged, *g_converged;
    int *f_calls, *g_calls, *mul_calls;
    int *status, *info;         /* lsq_status of the block; info: see above, -1 when there is none */
    int outer_iterations;       /* out: passes of the device loop = max over the blocks of iterations */
    double seconds;             /* out: wall time of the loop (host clock, includes syncs) */
    int trace_cap;              /* in: rows of the trace arrays (0: no trace) */
    double *trace_ssr, *trace_gnorm, *trace_delta, *trace_rho;   /* trace_cap * B */
    int *trace_accept;          /* trace_cap * B */
    double *trace_x;            /* trace_cap * n */
} lsq_batched_result;
int lsq_optimize_batched(lsq_ctx *ctx, int optimizer, int solver_kind, lsq_mat *J, double *d_x,
                         double *d_fcur, lsq_f_callback f, lsq_g_callback g, void *user,
                         const lsq_options *opt, void *batched_result);

/* ---- robust losses and observation weights: a wrapper around the problem ----
 * Measured data come with per-point uncertainties sigma_i and with outliers.  With z_i = f_i / sigma_i (z_i = f_i without
 * sigmas), a_i = |z_i| / c (c > 0: the loss scale) and a loss rho(s), s = a^2, the WRAPPED problem has
 *   the residual  r~_i = sign(z_i) c sqrt(rho(a_i^2))
 *   the Jacobian  J~ = diag(w_i / sigma_i) J,   w_i = d r~_i / d z_i = rho'(s) sqrt(s) / sqrt(rho(s)),  w_i = 1 at s = 0.
 * It is an exact least-squares problem: sum(abs2, r~) = c^2 sum(rho), twice the robust cost, and J~'r~ = J'(rho' f / sigma^2),
 * the exact gradient of that cost.  So the reference's accept ratio, convergence flags and ssr, every solver, lsq_optimize,
 * lsq_optimize_batched, g = NULL (central differences of the wrapped f ARE the Jacobian of r~) and every covariance entry
 * apply unchanged: at the solution a covariance entry sees J~ in the handle and r~ in d_fcur -- with LSQ_LOSS_LINEAR and sigmas
 * the textbook weighted covariance.  (Not the Triggs / scipy scaling, whose Jacobian carries a second-order correction and
 * whose residual scale is sqrt(rho'): that one is not the gradient of an exact sum of squares.)
 *   kind              r~                                                       w
 *   LSQ_LOSS_LINEAR   z                                                        1
 *   LSQ_LOSS_HUBER    a <= 1: z;  a > 1: q = sqrt(2a - 1) (2 sqrt(a / 2) when   1;  1 / q
 *                     a > 2^1022: 2a would overflow), copysign(c q, z)
 *   LSQ_LOSS_SOFT_L1  t = sqrt(1 + a a) (t = a when a > 2^500),                1 / (t q)
 *                     q = sqrt(2 / (t + 1)), z q
 *   LSQ_LOSS_CAUCHY   a < 2^-27: z.  Else L = log1p(a a) (2 log(a) when        1;  1 / ((1 + a a) q)
 *                     a > 2^500), q = sqrt(L) / a, z q                             ((1 / (a q)) / a when a > 2^500:
 *                                                                                  1 / a^2 would underflow)
 * Every operation of the table is one IEEE operation in that order; the row factor applied to J is w_i / sigma_i, one division.
 * Linear, Huber and soft-l1 give the bits of a host evaluation in that order (leastsquaresoptim.jl_amd/api.py: loss_transform);
 * Cauchy contains a log1p and agrees to rounding.  Signed zeros pass through; a NaN or an infinite f_i comes out as it went in
 * (w_i = 1 for NaN, 0 for +-Inf, except LSQ_LOSS_LINEAR: 1), so check_isfinite reports the index it would without a loss;
 * 0 <= w <= 1 and |r~| <= |z|.
 * lsq_loss_create: d_sigma_or_null is NULL or m device doubles, COPIED (the caller may free them); the object owns three
 * m-vectors (that copy, a raw residual, the row factors).  LSQ_EARG: an unknown kind, a scale that is not finite and positive,
 * a sigma that is not finite and positive (one readback at creation; the message names the index).  m < 1: LSQ_EDIM.
 * The handle is spelled void * for the reason lsq_optimize_batched spells its result so.
 * lsq_loss_eval: the transform itself, one elementwise kernel: d_f (m raw residuals) -> d_rt_or_null (r~; may be d_f itself) and
 * d_rowfactor_or_null (w / sigma), both in one pass.  h_stats_or_null: NULL (stream-ordered, nothing waits) or two host doubles:
 * [0] = sum(abs2, r~) through lsq_sumsq (the bits the loops compute), [1] = the number of rows with a > 1.
 * lsq_loss_set_problem gives the object the caller's own f! and g! (g_or_null = NULL: none) and their user pointer; then
 * lsq_optimize / lsq_optimize_batched / lsq_fd_jacobian are handed lsq_loss_f(), lsq_loss_g() -- or a null g for central
 * differences -- and the loss handle as `user`:
 *   lsq_loss_f  calls the inner f into d_out and transforms it in place;
 *   lsq_loss_g  calls the inner g, evaluates the inner f at the same d_x into the object's scratch (one evaluation the loop does
 *               not count, like the reference's finite-difference closure; nothing is cached from an earlier f call:
 *               lsq_optimize_batched hands g per-block points no f call has seen), derives the row factors and calls
 *               lsq_mat_scale_rows.
 * A failure inside either returns non-zero, so the loop reports LSQ_ECALLBACK, and lsq_last_error keeps the wrapper's reason
 * (the reason outlives the loop's generic "user callback reported failure" only; the next loop, solve or handle mutation
 * starts clean):
 * an inner callback failed, lsq_loss_set_problem was never called, J has another row count than m, or the handle is one
 * lsq_mat_scale_rows refuses.  The handle and the loss object stay usable afterwards.
 * Sharded and row-sharded runs (allreduce / row_allreduce in the options) with a loss are not covered. */
enum { LSQ_LOSS_LINEAR = 0, LSQ_LOSS_HUBER = 1, LSQ_LOSS_SOFT_L1 = 2, LSQ_LOSS_CAUCHY = 3 };
int lsq_loss_create(lsq_ctx *ctx, int kind, double scale, int m, const double *d_sigma_or_null, void **out);
int lsq_loss_destroy(void *loss);
int lsq_loss_set_problem(void *loss, lsq_f_callback f, lsq_g_callback g_or_null, void *user);
lsq_f_callback lsq_loss_f(void);      /* pass these with user = the loss handle */
lsq_g_callback lsq_loss_g(void);
int lsq_loss_eval(void *loss, const double *d_f, double *d_rt_or_null, double *d_rowfactor_or_null, double *h_stats_or_null);

/* ---- built-in device-side model for the synthetic benchmarks:
 *      r(x) = A tanh(x) - b,  J = A diag(1 - tanh(x)^2); A has J's pattern. ---- */
int lsq_model_tanh_create(lsq_ctx *ctx, lsq_mat *J, const double *h_Avalues, const double *h_b,
                          lsq_model **out);
int lsq_model_destroy(lsq_model *md);
lsq_f_callback lsq_model_f(void);
lsq_g_callback lsq_model_g(void);
/* what the solves on this model ran on.  sliced_rows / sliced_cols: 1 if J's sliced row / column layout is built.  lsmr_path:
 * lsq_solver_lsmr_path of the solver that the context's latest lsq_optimize on J kept (0: none, or the context has since
 * solved on another handle).  pair_tails: how often LM's tail took the predicted and the trial residual in one pass over A
 * (k_sell_rows_pair) since the model was created.  Read-only; the tests use it to know which kernels a model solve ran. */
int lsq_model_paths(const lsq_model *md, int *sliced_rows, int *sliced_cols, int *lsmr_path, long long *pair_tails);

/* ---- deterministic synthetic inputs (host side; counter-based RNG) ---- */
/* CSC with exactly `per_col` distinct sorted rows per column, values N(0,1)/sqrt(per_col). */
int lsq_synth_sparse(int m, int n, int per_col, unsigned long long seed, int *h_colptr,
                     int *h_rowval, double *h_nzval);
/* dense column-major N(0,1)/sqrt(m) */
int lsq_synth_dense(int m, int n, unsigned long long seed, double *h_values);
/* x_true ~ U(-1,1) (n) and noise ~ N(0,1) (m) streams */
int lsq_synth_uniform(int n, unsigned long long seed, double lo, double hi, double *h_out);
int lsq_synth_normal(int n, unsigned long long seed, double *h_out);

/* ---- measurement helpers ---- */
/* Times `reps` launches of y <- alpha*J*x + beta*y (trans=0) or the transpose (trans=1) with HIP
 * events on the context stream; returns the average milliseconds per launch. */
int lsq_bench_mul(lsq_mat *J, int trans, int reps, const double *d_x, double *d_y, double beta,
                  float *h_ms_per_launch);

/* A neighbour on the device, for tests and measurements of the paths above: `workgroups` workgroups of 256 threads, each
 * holding lds_bytes of LDS, spin for `milliseconds` on a stream of their own (returns at once; lsq_bench_occupy_wait joins). */
int lsq_bench_occupy(lsq_ctx *ctx, int workgroups, int lds_bytes, double milliseconds);
int lsq_bench_occupy_wait(lsq_ctx *ctx);

/* Reference-order arithmetic for small problems (m, n <= 2048, nnz <= 2^18): every sum is taken in
 * the order of the reference's serial loops, so iteration / mul counts reproduce the CPU
 * restatement exactly even where LSMR's stop iteration depends on the last bit.
 * on = 1 / 0 forces it on / off, -1 restores the default (on; env LSQ_EXACT=0 turns it off). */
int lsq_set_exact(int on);

/* Debug modes, process-wide (the hazard / serialised build the reference gets from Julia's --check-bounds and a
 * single thread; also environment LSQ_DEBUG_LAUNCH_JITTER=<us>, LSQ_DEBUG_SERIAL=<0|1|2>, read when the first context is made):
 *   launch_jitter_us > 0  random host stalls of up to that many microseconds (one in 64: 20x) in front of one kernel launch in
 *                         four -- any hand-off between kernels that holds only because the next launch follows at once breaks;
 *   serial = 1            every launch is waited for before the host goes on: no side-stream concurrency, no LSMR look-ahead,
 *                         no speculation -- SAME kernels and arithmetic, results must be bit-identical to the normal mode;
 *   serial = 2            additionally without the in-kernel workgroup exchanges (QR slab exchange, pipelined triangular
 *                         solves, one-launch Cholesky): the multi-launch fallbacks, equal to the fast paths to round-off.
 * A negative argument leaves that setting alone.  lsq_debug_get also reports the number of stalls injected so far. */
int lsq_debug_set(int launch_jitter_us, int serial);
int lsq_debug_get(int *launch_jitter_us, int *serial, long long *stalls);

/* HIP-event instrumentation of the two dominant kernels inside lsq_ldiv(_damped) with LSMR:
 * kernel 0 = K1 (u <- J t - cu u, the J*v product), kernel 1 = K2 (v <- J'u ..., the J'*u product).
 * Events are recorded on the context stream around each launch while enabled (up to max_samples
 * per kernel); lsq_prof_end waits for them and returns average milliseconds and sample counts. */
int lsq_prof_begin(lsq_ctx *ctx, int max_samples);
/* bit k of kernel_mask: instrument kernel k (default 3 = both).  A timed launch costs a few
 * microseconds of pipeline gaps, so bench.py times only kernel 0 inside the timed region. */
int lsq_prof_select(lsq_ctx *ctx, int kernel_mask);
int lsq_prof_end(lsq_ctx *ctx, double h_avg_ms[2], int h_count[2]);
/* average milliseconds between two HIP events recorded back to back with NOTHING in between: the
 * marker overhead contained in every bracketed interval above (for calibration). */
int lsq_prof_overhead(lsq_ctx *ctx, int pairs, double *h_ms);

#ifdef __cplusplus
}
#endif
#endif
