// lsq_optimize_batched: B independent fits on a block-diagonal Jacobian, one trust region PER BLOCK.
//
// For every block b this is the reference's optimize! (levenberg_marquardt.jl:39-144 / dogleg.jl:41-203 with Cholesky()) on
// the mb x nb problem made of residual rows b*mb .. and parameters b*nb ..: its own delta, decrease_factor / reuse flag, rho,
// accept decision, assess_convergence, iteration and call counts.  All of that state lives in device arrays of length B
// (BtDev); per outer iteration the host reads ONE 64-bit word back ({blocks still active, blocks that need their Jacobian})
// and never a per-block scalar.  The stream carries, besides g! / f!:
//   k_bd_solve (lsq_blockdiag.hip)  masked batched solve; LM's damping is formed inside from delta_b and the block's own
//                                   diag(J_b'J_b); J_b'fcur_b (the gradient) and the diagonal come out of the same pass
//   k_bt_step                       one wavefront per block: verdict of the solve, Dogleg's Cauchy / dogleg arithmetic
//                                   (dogleg.jl:85-145), box clip, trial point, max|dx_b|, projected gradient maximum
//   k_bt_decide                     one wavefront per block: sum(abs2, ftrial_b), sum(abs2, J_b dx_b - fcur_b), rho_b, accept,
//                                   assess_convergence, delta_b update, commit of x_b / fcur_b, trace row, next state
// A block is owned by one wavefront in every kernel and its sums are taken in a fixed order (lane-strided partial sums, then
// wave_sum), so the result for block b does not depend on B, on the other blocks or on the run: no floating-point atomics,
// no waits between workgroups (the only shared words are the two integer counters).
// J_b dx_b is formed by a block kernel of its own (bt_jv_sumsq), not by lsq_mul on the handle: the handle picks its product
// layout from the size of the WHOLE matrix (reference-order kernels, CSR segments, sliced rows), so a block's predicted
// residual would depend on how many other blocks share the batch.
#include <chrono>
#include <climits>

#include "lsq_loop.h"      // the trust-region constants

namespace {

struct BtDev {      // per-block state, device arrays of length B
    double *delta, *decf, *ssr, *ssr0, *maxdx, *maxgr, *wn_gn, *wn_gr, *alpha, *wn_dx;
    int *active, *solve, *needj, *reuse, *iter, *xc, *fc, *gc, *conv, *fcalls, *gcalls, *mcalls, *status, *info;
};
constexpr int BT_ND = 10, BT_NI = 14;

struct BtOpt {
    double x_tol, f_tol, g_tol, delta0;
    int iterations;
};

struct BtTrace {    // device mirrors of the caller's trace arrays (cap x B, x: cap x n); cap = 0: none
    int cap;
    double *ssr, *gnorm, *delta, *rho, *x;
    int *accept;
};

__device__ __forceinline__ int bt_wave_min(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = min(v, __shfl_xor(v, off));
    return v;
}

// first non-finite entry of the block's x (lane = entry), or -1: check_isfinite (utils.jl:70-75)
__device__ __forceinline__ int bt_first_nonfinite(double v, bool in, int lane) {
    const int k = bt_wave_min((in && !isfinite(v)) ? lane : INT_MAX);
    return k == INT_MAX ? -1 : k;
}

// sum over the block's rows of (J_b v - f_b)^2 (f == nullptr: of (J_b v)^2), every lane gets it.  v: this lane's entry of the
// nb-vector (column scale already applied).  Row r is owned by lane r % 64, columns in index order, then wave_sum.
__device__ __forceinline__ double bt_jv_sumsq(const double *__restrict__ vals, int mb, int nb, double v,
                                              const double *__restrict__ f, int lane) {
    double acc = 0.0;
    for (int r0 = 0; r0 < mb; r0 += 64) {
        const int r = r0 + lane;
        const bool ok = r < mb;
        double s = 0.0;
        for (int c = 0; c < nb; ++c) {
            const double vc = lsq_readlane_f64(v, c);
            const double a = ok ? vals[(size_t)c * mb + r] : 0.0;
            s += a * vc;
        }
        if (f && ok) s += -1.0 * f[r];
        acc += s * s;
    }
    return wave_sum(acc);
}

__device__ __forceinline__ double bt_sumsq(const double *__restrict__ f, int mb, int lane) {
    double acc = 0.0;
    for (int r = lane; r < mb; r += 64) acc += f[r] * f[r];
    return wave_sum(acc);
}

// levenberg_marquardt.jl:53-63 / dogleg.jl:58-69 per block, after the one f!(fcur, x0) of all blocks
template <bool LM>
__global__ void __launch_bounds__(256)
k_bt_init(int B, int mb, int nb, BtDev s, BtOpt o, const double *__restrict__ x, const double *__restrict__ fcur,
          double *__restrict__ xg, int *__restrict__ counts) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const bool in = lane < nb;
    const size_t j = (size_t)b * nb + (in ? lane : 0);
    const double xv = in ? x[j] : 0.0;
    if (in) xg[j] = xv;
    const double ssr = bt_sumsq(fcur + (size_t)b * mb, mb, lane);
    const int bad = bt_first_nonfinite(xv, in, lane);
    if (lane == 0) {
        const int act = (o.iterations > 0 && bad < 0) ? 1 : 0;
        s.delta[b] = o.delta0;
        s.decf[b] = 2.0;
        s.ssr[b] = s.ssr0[b] = ssr;
        s.maxdx[b] = 0.0;
        s.maxgr[b] = INFINITY;
        s.wn_gn[b] = s.wn_gr[b] = s.alpha[b] = s.wn_dx[b] = 0.0;
        s.active[b] = s.solve[b] = s.needj[b] = act;
        s.reuse[b] = 0;
        s.iter[b] = 0;
        s.xc[b] = s.fc[b] = s.gc[b] = s.conv[b] = 0;
        s.fcalls[b] = 1;
        s.gcalls[b] = s.mcalls[b] = 0;
        s.status[b] = (o.iterations > 0 && bad >= 0) ? LSQ_ENONFINITE : LSQ_OK;
        s.info[b] = (o.iterations > 0 && bad >= 0) ? bad : -1;
        if (act) {
            atomicAdd(&counts[0], 1);
            atomicAdd(&counts[1], 1);
        }
    }
}

// From the solve to the trial point.  LM: levenberg_marquardt.jl:87-106 (dx holds the solve's output on entry);
// Dogleg: dogleg.jl:85-160 (sol = the Gauss-Newton step of the blocks that were solved in this iteration).
template <bool LM>
__global__ void __launch_bounds__(256)
k_bt_step(int B, int mb, int nb, BtDev s, bool qr, const double *__restrict__ vals, const double *__restrict__ scale,
          const int *__restrict__ binfo, const double *__restrict__ grad, const double *__restrict__ diag,
          double *__restrict__ dtd, double *__restrict__ dgr, const double *__restrict__ dgn, const double *__restrict__ x,
          const double *__restrict__ lo, const double *__restrict__ hi, double *__restrict__ dx, double *__restrict__ xt) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const bool in = lane < nb;
    const size_t j = (size_t)b * nb + (in ? lane : 0);
    const double xv = in ? x[j] : 0.0;
    if (!s.active[b]) {        // frozen: its entries of the trial point are its final x_b
        if (in) { xt[j] = xv; dx[j] = 0.0; }
        return;
    }
    const int iter = s.iter[b] + 1;
    const bool fresh = LM ? true : s.reuse[b] == 0;      // the block was solved in this iteration
    const int needj = LM ? s.needj[b] : (fresh ? 1 : 0);
    if (qr) {                  // BlockQR(): no block fails on rank; binfo[b] is the rank of the solve
        if (fresh && lane == 0) s.info[b] = binfo[b];
    } else if (fresh && binfo[b] != 0) {
        // dense_cholesky.jl:57 PosDefException / :33 RankDeficientException of THIS block: frozen with the iterate it holds;
        // the counts are those of the reference at the throw (iter, g!; Dogleg: the two products in front of the solve)
        if (in) { xt[j] = xv; dx[j] = 0.0; }
        if (lane == 0) {
            s.status[b] = LM ? LSQ_ENOTPD : LSQ_ERANK;
            s.info[b] = LM ? binfo[b] : nb - binfo[b];
            s.iter[b] = iter;
            s.gcalls[b] += needj;
            if (!LM) s.mcalls[b] += 2;
            s.active[b] = 0;
        }
        return;
    }
    double d, maxgr = s.maxgr[b], wn_dx = 0.0;
    if (LM) {
        d = in ? dx[j] : 0.0;
        double gi = in ? grad[j] : 0.0;                                           // :102
        if (lo && in && xv <= lo[j] && gi > 0.0) gi = 0.0;                        // utils.jl:39-55
        else if (hi && in && xv >= hi[j] && gi < 0.0) gi = 0.0;
        maxgr = wave_max(fabs(gi));
    } else {
        double delta = s.delta[b], tdt, gr, gn, wn_gn, wn_gr, alpha;
        if (fresh) {
            const double cs = in ? diag[j] : 0.0;                                 // :85
            tdt = in ? (cs > MAX_DIAGONAL ? MAX_DIAGONAL : (cs < MIN_DIAGONAL ? MIN_DIAGONAL : cs)) : 0.0;   // :90
            if (iter == 1) {                                                      // :92-97
                const double wx = sqrt(wave_sum(tdt * xv * xv));
                if (wx > 0.0) delta *= wx;
            }
            const double g = in ? grad[j] : 0.0;                                  // :99
            double gi = g;
            if (lo && in && xv <= lo[j] && gi > 0.0) gi = 0.0;
            else if (hi && in && xv >= hi[j] && gi < 0.0) gi = 0.0;
            maxgr = wave_max(fabs(gi));
            gr = in ? g / tdt : 0.0;                                              // :105
            wn_gr = sqrt(wave_sum(tdt * gr * gr));                                // :106
            const double sc = (scale && in) ? scale[j] : 1.0;
            const double jg = bt_jv_sumsq(vals + (size_t)b * mb * nb, mb, nb, gr * sc, nullptr, lane);   // :109
            alpha = wn_gr * wn_gr / jg;                                           // :111
            gn = in ? dgn[j] : 0.0;                                               // :115
            wn_gn = sqrt(wave_sum(tdt * gn * gn));                                // :117
            if (in) { dtd[j] = tdt; dgr[j] = gr; }
        } else {
            tdt = in ? dtd[j] : 0.0;
            gr = in ? dgr[j] : 0.0;
            gn = in ? dgn[j] : 0.0;
            wn_gn = s.wn_gn[b]; wn_gr = s.wn_gr[b]; alpha = s.alpha[b];
        }
        if (wn_gn <= delta) {                                                     // :120 case 1
            d = gn;
            wn_dx = wn_gn;
        } else if (wn_gr * alpha >= delta) {                                      // :124 case 2
            d = gr * (delta / wn_gr);
            wn_dx = delta;
        } else {                                                                  // :131 case 3
            const double b_dot_a = alpha * wave_sum(tdt * gr * gn);
            const double a2 = (alpha * wn_gr) * (alpha * wn_gr);
            const double bma2 = a2 - 2 * b_dot_a + wn_gn * wn_gn;
            const double cc = b_dot_a - a2;
            const double q = sqrt(cc * cc + bma2 * (delta * delta - a2));
            const double beta = (cc <= 0) ? (q - cc) / bma2 : (delta * delta - a2) / (q + cc);
            d = gn * beta;
            d += (alpha * (1 - beta)) * gr;
            wn_dx = sqrt(wave_sum(tdt * d * d));                                  // :144
        }
        if (lane == 0) {
            s.delta[b] = delta;
            s.wn_gn[b] = wn_gn; s.wn_gr[b] = wn_gr; s.alpha[b] = alpha;
            if (fresh) s.mcalls[b] += 3;
        }
    }
    // levenberg_marquardt.jl:89-98.  Julia's min / max propagate NaN from EITHER argument (fmin / fmax drop it): a NaN step
    // component must stay NaN so that the block's trial point is non-finite, as k_box_clip keeps it for a single fit
    if (lo && in) { const double a = xv - lo[j]; d = (d != d || a != a) ? d + a : (d < a ? d : a); }
    if (hi && in) { const double a = xv - hi[j]; d = (d != d || a != a) ? d + a : (d > a ? d : a); }
    const double maxdx = wave_max(d != d ? INFINITY : fabs(d));     // maximum(abs, dx): a NaN fails "<= x_tol", as in lsq_vec.hip
    if (in) {
        dx[j] = d;
        xt[j] = xv + -1.0 * d;                                                    // axpy!(-1, dx, x)
    }
    if (lane == 0) {
        s.iter[b] = iter;
        s.gcalls[b] += needj;
        s.maxdx[b] = maxdx;
        s.maxgr[b] = maxgr;
        s.wn_dx[b] = wn_dx;
    }
}

// levenberg_marquardt.jl:107-139 / dogleg.jl:164-198 per block, then the block's state for the next outer iteration
template <bool LM>
__global__ void __launch_bounds__(256)
k_bt_decide(int B, int mb, int nb, BtDev s, BtOpt o, const double *__restrict__ vals, const double *__restrict__ scale,
            double *__restrict__ x, const double *__restrict__ xt, const double *__restrict__ dx, double *__restrict__ fcur,
            const double *__restrict__ ftrial, double *__restrict__ xg, BtTrace tr, int *__restrict__ counts) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    if (!s.active[b]) return;          // frozen: nothing of it changes, whatever f! wrote into its rows of ftrial
    const bool in = lane < nb;
    const size_t j = (size_t)b * nb + (in ? lane : 0);
    const double d = in ? dx[j] : 0.0;
    const double sc = (scale && in) ? scale[j] : 1.0;
    double *fb = fcur + (size_t)b * mb;
    const double *ft = ftrial + (size_t)b * mb;
    const double trial_ssr = bt_sumsq(ft, mb, lane);
    const double predicted_ssr = bt_jv_sumsq(vals + (size_t)b * mb * nb, mb, nb, d * sc, fb, lane);
    double ssr = s.ssr[b], delta = s.delta[b];
    const double pred_red = fabs(ssr - predicted_ssr);
    const double rho = pred_red > 0 ? (ssr - trial_ssr) / pred_red : 0.0;
    const bool accepted = LM ? rho > MIN_STEP_QUALITY : rho >= MIN_STEP_QUALITY;
    int xc = 0, fc = 0, gc = 0;        // utils.jl:7-31
    if (accepted && fabs(trial_ssr - ssr) <= o.f_tol * (fabs(ssr) + o.f_tol)) fc = 1;
    else if (s.maxdx[b] <= o.x_tol) xc = 1;
    else if (s.maxgr[b] <= o.g_tol) gc = 1;
    const int conv = xc | fc | gc;
    double decf = s.decf[b];
    double xn;
    if (accepted) {
        xn = in ? xt[j] : 0.0;
        for (int r = lane; r < mb; r += 64) fb[r] = ft[r];
        ssr = trial_ssr;
    } else {
        xn = in ? xt[j] + 1.0 * d : 0.0;                                          // axpy!(1, dx, x): (x - dx) + dx
    }
    if (LM) {
        if (accepted) {
            const double t = 2.0 * rho - 1.0;
            const double q = 1.0 - t * t * t;
            const double dn = delta / (1.0 / 3.0 > q ? 1.0 / 3.0 : q);            // :130
            delta = dn < MAX_DELTA ? dn : MAX_DELTA;
            decf = 2.0;
        } else {
            const double dn = delta / decf;
            delta = dn > MIN_DELTA ? dn : MIN_DELTA;
            decf *= 2.0;
        }
    } else {
        if (rho < DECREASE_THRESHOLD) {                                           // dogleg.jl:193-197
            const double dn = delta * 0.5;
            delta = dn > MIN_DELTA ? dn : MIN_DELTA;
        } else if (rho > INCREASE_THRESHOLD) {
            const double dn = 3.0 * s.wn_dx[b];
            delta = delta > dn ? delta : dn;
        }
    }
    if (in) x[j] = xn;
    const int iter = s.iter[b];
    if (tr.cap > 0 && iter <= tr.cap) {
        const size_t k = (size_t)(iter - 1);
        if (in) tr.x[k * ((size_t)B * nb) + j] = xn;
        if (lane == 0) {
            tr.ssr[k * B + b] = ssr;
            tr.gnorm[k * B + b] = s.maxgr[b];
            tr.delta[k * B + b] = delta;
            tr.rho[k * B + b] = rho;
            tr.accept[k * B + b] = accepted ? 1 : 0;
        }
    }
    int status = LSQ_OK, info = -1, act = 1;
    if (conv || iter >= o.iterations) act = 0;
    else {
        const int bad = bt_first_nonfinite(xn, in, lane);                         // check_isfinite at the top of the next iteration
        if (bad >= 0) { act = 0; status = LSQ_ENONFINITE; info = bad; }
    }
    const int needj = act && accepted;
    if (needj && in) xg[j] = xn;       // (else xg_b stays the point at which J_b was last evaluated)
    if (lane == 0) {
        s.ssr[b] = ssr;
        s.delta[b] = delta;
        s.decf[b] = decf;
        s.xc[b] = xc; s.fc[b] = fc; s.gc[b] = gc; s.conv[b] = conv;
        s.fcalls[b] += 1;
        s.mcalls[b] += LM ? 3 : 1;
        s.active[b] = act;
        s.needj[b] = needj;
        s.reuse[b] = accepted ? 0 : 1;
        s.solve[b] = LM ? act : needj;
        if (status != LSQ_OK) { s.status[b] = status; s.info[b] = info; }
        if (act) {
            atomicAdd(&counts[0], 1);
            if (needj) atomicAdd(&counts[1], 1);
        }
    }
}

struct BtBuffers {
    hipStream_t stream;
    double *dpool = nullptr, *tpool = nullptr;
    int *ipool = nullptr, *tipool = nullptr;
    ~BtBuffers() {     // (every exit, the failing ones included: nothing queued may still use the buffers)
        (void)hipStreamSynchronize(stream);
        hipFree(dpool); hipFree(tpool); hipFree(ipool); hipFree(tipool);
    }
};

template <bool LM>
int bt_loop(lsq_ctx *c, lsq_mat *J, bool qr, double *x, double *fcur, lsq_f_callback f, lsq_g_callback g, void *user,
            const lsq_options *o, lsq_batched_result *r) {
    const int B = J->bd_blocks, mb = J->bd_mb, nb = J->bd_nb, m = J->m, n = J->n;
    BtBuffers buf{c->stream};
    // doubles: state | xt dx xg grad diag dtd dgr dgn lo hi (n each) | ftrial (m)
    const size_t nd = (size_t)BT_ND * B + (size_t)10 * n + m;
    const size_t ni = (size_t)(BT_NI + 1) * B + 2;
    LSQ_HIP(hipMalloc(&buf.dpool, nd * sizeof(double)));
    LSQ_HIP(hipMalloc(&buf.ipool, ni * sizeof(int)));
    LSQ_HIP(hipMemsetAsync(buf.dpool, 0, nd * sizeof(double), c->stream));
    LSQ_HIP(hipMemsetAsync(buf.ipool, 0, ni * sizeof(int), c->stream));
    BtDev s;
    double **dp[BT_ND] = {&s.delta, &s.decf, &s.ssr, &s.ssr0, &s.maxdx, &s.maxgr, &s.wn_gn, &s.wn_gr, &s.alpha, &s.wn_dx};
    for (int k = 0; k < BT_ND; ++k) *dp[k] = buf.dpool + (size_t)k * B;
    int **ip[BT_NI] = {&s.active, &s.solve, &s.needj, &s.reuse, &s.iter, &s.xc, &s.fc, &s.gc, &s.conv, &s.fcalls, &s.gcalls,
                       &s.mcalls, &s.status, &s.info};
    for (int k = 0; k < BT_NI; ++k) *ip[k] = buf.ipool + (size_t)k * B;
    int *binfo = buf.ipool + (size_t)BT_NI * B, *counts = binfo + B;
    double *v = buf.dpool + (size_t)BT_ND * B;
    double *xt = v, *dx = v + n, *xg = v + 2 * (size_t)n, *grad = v + 3 * (size_t)n, *diag = v + 4 * (size_t)n,
           *dtd = v + 5 * (size_t)n, *dgr = v + 6 * (size_t)n, *dgn = v + 7 * (size_t)n, *lo = nullptr, *hi = nullptr;
    double *ftrial = v + 10 * (size_t)n;
    if (o->h_lower) {
        lo = v + 8 * (size_t)n;
        LSQ_HIP(hipMemcpyAsync(lo, o->h_lower, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    if (o->h_upper) {
        hi = v + 9 * (size_t)n;
        LSQ_HIP(hipMemcpyAsync(hi, o->h_upper, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    BtTrace tr{0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const int cap = r->trace_cap > 0 ? r->trace_cap : 0;
    const bool tracing = cap > 0 && r->trace_ssr && r->trace_gnorm && r->trace_delta && r->trace_rho && r->trace_accept && r->trace_x;
    if (tracing) {
        const size_t cb = (size_t)cap * B, cn = (size_t)cap * n;
        LSQ_HIP(hipMalloc(&buf.tpool, (4 * cb + cn) * sizeof(double)));
        LSQ_HIP(hipMalloc(&buf.tipool, cb * sizeof(int)));
        LSQ_HIP(hipMemsetAsync(buf.tpool, 0, (4 * cb + cn) * sizeof(double), c->stream));
        LSQ_HIP(hipMemsetAsync(buf.tipool, 0, cb * sizeof(int), c->stream));
        tr = BtTrace{cap, buf.tpool, buf.tpool + cb, buf.tpool + 2 * cb, buf.tpool + 3 * cb, buf.tpool + 4 * cb, buf.tipool};
    }
    BtOpt bo{o->x_tol, o->f_tol, o->g_tol, o->delta > 0 ? o->delta : (LM ? 10.0 : 1.0), o->iterations};
    const dim3 grid((B + 3) / 4), blk(256);

    if (f(fcur, x, user) != 0) { lsq_set_error("user callback reported failure"); return LSQ_ECALLBACK; }
    LSQ_LAUNCH(k_bt_init<LM>, grid, blk, 0, c->stream, B, mb, nb, s, bo, (const double *)x, (const double *)fcur, xg, counts);
    LSQ_HIP(hipGetLastError());
    int outer = 0;
    for (;;) {
        int cnt[4] = {0, 0, 0, 0};     // the iteration's one word: {active blocks, blocks whose Jacobian is wanted}
        LSQ_TRY(lsq_read_ints(c, counts, counts + 1, nullptr, nullptr, cnt));
        if (cnt[0] == 0) break;
        ++outer;
        // g! sees, for every block that does not want its Jacobian, the x_b at which it was last evaluated (xg), so a
        // deterministic g! rewrites the same J_b: the reference does not re-evaluate J_b at a reverted iterate, which may
        // differ from that point in the last bit (levenberg_marquardt.jl:135)
        if (cnt[1] > 0) LSQ_TRY(lsq_call_g(g, J, xg, user));
        LSQ_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int), c->stream));
        if (qr) LSQ_TRY(lsq_blockqr_solve_blocks(c, J, LM, fcur, s.delta, LM ? dx : dgn, s.solve, binfo, grad, diag));
        else LSQ_TRY(lsq_blockdiag_solve_blocks(c, J, !LM, fcur, s.delta, LM ? dx : dgn, s.solve, binfo, grad, diag));
        const double *vals = J->csc.d_val, *scale = J->d_colscale;
        LSQ_LAUNCH(k_bt_step<LM>, grid, blk, 0, c->stream, B, mb, nb, s, qr, vals, scale, (const int *)binfo, (const double *)grad,
                   (const double *)diag, dtd, dgr, (const double *)dgn, (const double *)x, (const double *)lo, (const double *)hi,
                   dx, xt);
        LSQ_HIP(hipGetLastError());
        if (f(ftrial, xt, user) != 0) { lsq_set_error("user callback reported failure"); return LSQ_ECALLBACK; }
        LSQ_LAUNCH(k_bt_decide<LM>, grid, blk, 0, c->stream, B, mb, nb, s, bo, vals, scale, x, (const double *)xt,
                   (const double *)dx, fcur, (const double *)ftrial, xg, tr, counts);
        LSQ_HIP(hipGetLastError());
    }
    // per-block results, once
    std::vector<double> hd((size_t)BT_ND * B);
    std::vector<int> hi_((size_t)BT_NI * B);
    LSQ_HIP(hipMemcpyAsync(hd.data(), buf.dpool, hd.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    LSQ_HIP(hipMemcpyAsync(hi_.data(), buf.ipool, hi_.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (tracing) {
        const size_t cb = (size_t)cap * B, cn = (size_t)cap * n;
        LSQ_HIP(hipMemcpyAsync(r->trace_ssr, tr.ssr, cb * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        LSQ_HIP(hipMemcpyAsync(r->trace_gnorm, tr.gnorm, cb * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        LSQ_HIP(hipMemcpyAsync(r->trace_delta, tr.delta, cb * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        LSQ_HIP(hipMemcpyAsync(r->trace_rho, tr.rho, cb * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        LSQ_HIP(hipMemcpyAsync(r->trace_accept, tr.accept, cb * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        LSQ_HIP(hipMemcpyAsync(r->trace_x, tr.x, cn * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    LSQ_HIP(hipStreamSynchronize(c->stream));
    auto col = [&](int k) { return hi_.data() + (size_t)k * B; };
    for (int b = 0; b < B; ++b) {
        if (r->ssr) r->ssr[b] = hd[(size_t)2 * B + b];
        if (r->ssr0) r->ssr0[b] = hd[(size_t)3 * B + b];
        if (r->iterations) r->iterations[b] = col(4)[b];
        if (r->x_converged) r->x_converged[b] = col(5)[b];
        if (r->f_converged) r->f_converged[b] = col(6)[b];
        if (r->g_converged) r->g_converged[b] = col(7)[b];
        if (r->converged) r->converged[b] = col(8)[b];
        if (r->f_calls) r->f_calls[b] = col(9)[b];
        if (r->g_calls) r->g_calls[b] = col(10)[b];
        if (r->mul_calls) r->mul_calls[b] = col(11)[b];
        if (r->status) r->status[b] = col(12)[b];
        if (r->info) r->info[b] = col(13)[b];
    }
    r->outer_iterations = outer;
    return LSQ_OK;
}

}  // namespace

// B runs of optimize! (levenberg_marquardt.jl:39-144 / dogleg.jl:41-203, Cholesky(): dense_cholesky.jl:29-59) in one device loop
extern "C" int lsq_optimize_batched(lsq_ctx *c, int optimizer, int solver_kind, lsq_mat *J, double *x, double *fcur,
                                    lsq_f_callback f, lsq_g_callback g, void *user, const lsq_options *opt, void *result) {
    LSQ_RANGE("lsq_optimize_batched");
    lsq_batched_result *res = (lsq_batched_result *)result;
    if (!c || !J || !x || !fcur || !f || !opt || !res) {
        lsq_set_error("lsq_optimize_batched: null argument");
        return LSQ_EARG;
    }
    res->outer_iterations = 0;
    res->seconds = 0.0;
    if (optimizer != LSQ_LEVENBERG_MARQUARDT && optimizer != LSQ_DOGLEG) {
        lsq_set_error("lsq_optimize_batched: unknown optimizer %d", optimizer);
        return LSQ_EARG;
    }
    if (solver_kind == LSQ_SCHUR) {
        lsq_set_error("lsq_optimize_batched: Schur() solves the one coupled system of a bordered block-diagonal Jacobian, there is "
                      "no trust region per block in it. Use lsq_optimize with LevenbergMarquardt");
        return LSQ_EARG;
    }
    if (solver_kind == LSQ_BORDERED_QR) {
        lsq_set_error("lsq_optimize_batched: BorderedQR() solves the one coupled system of a bordered block-diagonal Jacobian, "
                      "there is no trust region per block in it. Use lsq_optimize with LevenbergMarquardt");
        return LSQ_EARG;
    }
    if (J->kind != LSQ_MAT_CSC || J->bd_blocks < 1) {
        lsq_set_error("lsq_optimize_batched: the Jacobian is not block-diagonal (lsq_blockdiag_create): one trust region per "
                      "block needs the block shape");
        return LSQ_EARG;
    }
    if (solver_kind == LSQ_QR) {
        lsq_set_error("solver QR() is not available for sparse Jacobians. Choose between Cholesky() and LSMR()");
        return LSQ_EARG;
    }
    if (solver_kind == LSQ_LSMR) {
        lsq_set_error("lsq_optimize_batched: LSMR() is not available per block (an iterative solve per block is a different "
                      "loop). Use Cholesky(), or lsq_optimize for one trust region over the stacked problem");
        return LSQ_EARG;
    }
    if (solver_kind != LSQ_CHOLESKY && solver_kind != LSQ_BLOCK_QR) {
        lsq_set_error("lsq_optimize_batched: unknown solver %d", solver_kind);
        return LSQ_EARG;
    }
    const bool qr = solver_kind == LSQ_BLOCK_QR;
    if (qr && J->bd_nb > 64) {
        lsq_set_error("lsq_optimize_batched: BlockQR() needs blocks of at most 64 columns (got %d blocks of %d x %d): one "
                      "block's triangular factor must fit the in-LDS factorisation", J->bd_blocks, J->bd_mb, J->bd_nb);
        return LSQ_EARG;
    }
    if (J->bd_nb > 64) {
        lsq_set_error("lsq_optimize_batched: Cholesky() per block needs blocks of at most 64 columns (got nb = %d): one block's "
                      "normal matrix must fit the 64 x 64 in-LDS factorisation", J->bd_nb);
        return LSQ_EARG;
    }
    if (opt->allreduce || opt->row_allreduce) {
        lsq_set_error("lsq_optimize_batched: sharded runs (lsq_options.allreduce / row_allreduce) are not available with one "
                      "trust region per block");
        return LSQ_EARG;
    }
    if (opt->preconditioner || opt->precond_update || opt->precond_ldiv) {
        lsq_set_error("lsq_optimize_batched: preconditioner hooks belong to LSMR(); the per-block loop solves with Cholesky()");
        return LSQ_EARG;
    }
    // g == NULL: g! is the central-difference Jacobian of f! (types.jl:54-58), nb colours whatever B is.  It is handed xg like
    // any g! and rewrites every block: a block that did not want its Jacobian gets the bits it already holds
    LsqFdCall fd{f, user, LSQ_OK};
    if (!g) {
        LSQ_TRY(lsq_fd_check(J, "lsq_optimize_batched without g!"));
        f = lsq_fd_f_thunk;
        g = lsq_fd_g_thunk;
        user = &fd;
    }
    LSQ_HIP(hipSetDevice(c->device));
    const int n = J->n;
    if (opt->h_lower || opt->h_upper) {        // levenberg_marquardt.jl:49-51 / dogleg.jl:52-54
        std::vector<double> hx(n);
        LSQ_TRY(lsq_d2h(c, hx.data(), x, (size_t)n * sizeof(double)));
        for (int i = 0; i < n; ++i)
            if ((opt->h_lower && !(hx[i] >= opt->h_lower[i])) || (opt->h_upper && !(hx[i] <= opt->h_upper[i]))) {
                lsq_set_error("ArgumentError: Initial guess must be within bounds.");
                return LSQ_EBOUNDS;
            }
    }
    auto t0 = std::chrono::steady_clock::now();
    int st = optimizer == LSQ_LEVENBERG_MARQUARDT ? bt_loop<true>(c, J, qr, x, fcur, f, g, user, opt, res)
                                                  : bt_loop<false>(c, J, qr, x, fcur, f, g, user, opt, res);
    hipStreamSynchronize(c->stream);
    if (st == LSQ_ECALLBACK && fd.status != LSQ_OK) st = fd.status;    // (what the central differences themselves ran into)
    res->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return st;
}
