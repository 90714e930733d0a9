// What crosses between the trust-region loops (lsq_optimize.hip) and the built-in tanh model (lsq_model.hip): the scalar slots,
// the constants that shape trajectories, and the hooks by which the loops let the model fuse its passes into theirs.  Internal
// like lsq_call_g and lsq_workspace_free: nothing here is part of include/lsqhip.h.
#pragma once
#include "lsq_solver.h"

// constants that shape trajectories (types.jl:107-111, dogleg.jl:38-39)
static constexpr double MIN_DELTA = 1e-16, MAX_DELTA = 1e16, MIN_STEP_QUALITY = 1e-3;
static constexpr double MIN_DIAGONAL = 1e-6, MAX_DIAGONAL = 1e32;
static constexpr double DECREASE_THRESHOLD = 0.25, INCREASE_THRESHOLD = 0.75;

// scalar slots used by the loops (ctx->d_slots); SL_SSR is the pair kernel's own (model_pair_tail)
enum { SL_GRAD = 8, SL_DX = 9, SL_NONFIN = 10, SL_TRIAL = 11, SL_PRED = 12, SL_SSR = 13, SL_W0 = 14, SL_W1 = 15,
       SL_W2 = 16, SL_SUM = 17 };

// grid of an n-length streaming launch
static inline int ngrid(const lsq_ctx *c, long long n) {
    long long g = (n + LSQ_NT - 1) / LSQ_NT;
    long long cap = (long long)c->num_cus * 8;
    if (g > cap) g = cap;
    return g < 1 ? 1 : (int)g;
}

// Are the callbacks the built-in model's: f! (and g!, where the caller names it)?  What only hands f! its buffers or takes its
// fused passes asks about f alone; what relies on g! installing the factors the step kernel has put into d_sspec asks about
// both -- lsq_model_f() is a public export and may be paired with somebody else's g!.
bool model_is_builtin(lsq_f_callback f, lsq_g_callback g = nullptr);

// f! + sum(abs2, out) -> slot in one pass (sliced rows only; *done tells whether it applied, else f! alone has run)
// mirror: the caller expects model_pair_tail to read `out` next -- the pass leaves it in slice order too (no k_sell_perm_rows)
int model_f_sumsq(void *user, double *out, const double *x, int ctr, double *d_out, LsqSlotPublish pub, bool *done,
                  const int *skip = nullptr, bool mirror = false);
// the start point of a solve on the model's sliced rows: tanh(x0), 1 - tanh(x0)^2 and the first non-finite index of x0 (-> slot)
// in one launch; *done tells whether it applied (else nothing was launched)
int model_start_point(void *user, const double *x, double *d_nonfin, bool *done);
// an error return between model_start_point and the g! that would have consumed its factors: nothing stays recorded
void model_forget_point(void *user);
// predicted residual |J dx - f|^2 AND f!(x_trial) with its sum of squares in ONE pass over the model's matrix
// (k_sell_rows_pair, lsq_sell.h); *done tells whether it applied (else nothing was launched: the caller takes the two passes)
// sg (optional): also queue the NEXT iteration's gradient + colsumabs2 pass behind it, guarded by the acceptance and convergence
// tests the kernel takes on the device (lsq_sparse_grad_colsum_spec); sg->launched tells whether that pass was queued
struct SpecGrad {
    int *gate;          // this pass's skip word (non-zero until the pair kernel clears it)
    double ssr;         // the current sum of squares (what the host will test rho against)
    double *grad;       // where the gradient goes
    bool launched;
    double xtol, ftol, gtol;    // the loop's tolerances (what the host's assess() will test with)
};
int model_pair_tail(void *user, lsq_mat *J, const double *dx, const double *fcur, double *ftrial, const double *xt,
                    double *slot_pred, double *slot_trial, LsqSlotPublish pub, const int *skip, bool *done,
                    SpecGrad *sg = nullptr);
// buffers for tanh(xt) and 1 - tanh(xt)^2 when the model's next f!(., xt) can take them from the step kernel (else nulls)
void model_trial_buffers(void *user, const double *xt, double **t_out, double **s_out);

// the other way (lsq_model_paths): the LSMR path last taken by the solver that lsq_optimize caches for J on this context (0: none)
int lsq_workspace_lsmr_path(const lsq_ctx *c, const lsq_mat *J);
