// Device-resident LSMR (Fong & Saunders) on the damped, Jacobi-preconditioned operator
//     A = [J; diag(sqrt(damp))] * diag(P)          b = (y, 0)
// replacing lsmr.jl:53-238 driven by iterative_lsmr.jl:179-198 (Dogleg) / :238-259 (LM).
//
// One inner iteration = three launches, zero host synchronisations:
//   K1  u~ <- J t - cu*u~   (+ damped rows, + sum u~^2 -> beta)          t = P.*v, cu = alpha/beta
//   K2  v~ <- P.*(J'u~ + d.*ux~)/beta - beta*v  (+ sum v~^2 -> alpha, + the two Givens chains,
//        ||r||, ||A||, cond(A) estimates: ~60 scalar flops in the last block)
//   K3  v <- v~/alpha; hbar, x, h updates; t <- P.*v; sum x^2 -> ||x||; the 7 stopping rules
// The PreconditionedMatrix / DampenedMatrix / MyAdjoint / InverseDiagonal wrappers
// (iterative_lsmr.jl:12-122) become epilogue arithmetic; u is kept UNNORMALISED (its 1/beta is
// folded into the consumer), which removes the rmul! passes over the m-vector (lsmr.jl:121).
// The recurrence lives in device memory; the host learns about termination through a pinned
// mailbox word and runs at most LSQ_LOOKAHEAD_DEFAULT iterations ahead (kernels of a finished solve exit
// on their first instruction).  Stopping rules are evaluated every iteration, so `iter` (and
// mul_calls = 2*iter, lsmr.jl:236) is the count the reference would report.
#include <chrono>
#include <cmath>
#include <cstdlib>

#include "lsq_solver.h"
#include "lsq_spmv.h"

static constexpr int LSQ_LOOKAHEAD_DEFAULT = 2;

// mailbox word: [63:41] epoch | [40] done | [39:32] istop | [31:0] iter
__device__ __forceinline__ void publish(LsqMailbox *mail, const LsmrState *st) {
    unsigned long long w = ((unsigned long long)(st->epoch & 0x7fffffu) << 41) |
                           ((unsigned long long)(st->done ? 1 : 0) << 40) |
                           ((unsigned long long)(st->istop & 0xff) << 32) | (unsigned)st->iter;
    __hip_atomic_store((unsigned long long *)mail, w, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- setup: P, sqrt(damp) (iterative_lsmr.jl:129-141, 251-252) ------------------------------
__global__ void __launch_bounds__(LSQ_NT)
k_lsmr_prep(int n, const double *__restrict__ colsum, double *__restrict__ damp, double *__restrict__ P,
            double *__restrict__ dg, double *__restrict__ ux, int custom_p) {
    for (int j = blockIdx.x * LSQ_NT + threadIdx.x; j < n; j += gridDim.x * LSQ_NT) {
        double s = colsum[j];
        if (damp) {
            double d = damp[j];
            s += d;                  // axpy!(1, damp, out._)  -- damp is still dtd/Delta here
            double r = sqrt(d);      // map!(sqrt, damp, damp)
            dg[j] = r;
            damp[j] = r;             // the reference clobbers the caller's damp (:252)
            ux[j] = 0.0;             // zerosvector (:246)
        }
        if (!custom_p) P[j] = s > 0.0 ? 1.0 / sqrt(s) : 0.0;   // (custom_p: the caller's preconditioner! filled P)
    }
}

// ---- beta_1^2 = sum(b^2) as block partials, and state reset (lsmr.jl:73-75 with x == 0) --------
__global__ void __launch_bounds__(LSQ_NT)
k_lsmr_begin(int m, const double *__restrict__ y, LsmrState *st, double *pu, int *npu, double atol, double btol,
             double ctol, int maxiter, unsigned epoch) {
    __shared__ double sh[LSQ_NT / 64];
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // no other kernel touches the state concurrently
        st->iter = 0;
        st->istop = 0;
        st->done = 0;
        st->notdone = 1;
        st->first = 1;
        st->atol = atol;
        st->btol = btol;
        st->ctol = ctol;
        st->maxiter = maxiter;
        st->epoch = epoch;
        st->cu = 0.0;
        *npu = (int)gridDim.x;
    }
    double acc = 0.0;
    for (long long i = blockIdx.x * (long long)LSQ_NT + threadIdx.x; i < m; i += (long long)gridDim.x * LSQ_NT) {
        double v = y[i];
        acc += v * v;
    }
    double bv = block_sum<LSQ_NT>(acc, sh);
    if (threadIdx.x == 0) pu[blockIdx.x] = bv;
}

// ---- K1: u~ <- J t - cu u~ ; publishes the block partials of sum(u~^2) --------------------------
struct EpiU {
    static constexpr bool REDUCE = true;
    using defer = void;
    const int *done;
    int extra_blocks;
    LsmrState *st;
    const double *uold;
    double *unew;
    // damped rows
    int n;
    const double *dg;
    const double *t;
    double *ux;
    double *partials;   // pu
    int *npartials;
    unsigned *counter;  // unused (deferred)
    double cu;          // cached st->cu
    using has_prepare = void;
    __device__ void prepare() { cu = st->cu; }
    __device__ void seg(int s, double dot, double &racc) const {
        double un = dot - st->cu * uold[s];
        unew[s] = un;
        racc += un * un;
    }
    using has_pre = void;
    __device__ double pre(int s) const { return uold[s]; }
    __device__ void seg_pre(int s, double dot, double uo, double &racc) const {
        double un = dot - cu * uo;
        unew[s] = un;
        racc += un * un;
    }
    __device__ void extra(int, double &) const {}   // (the damped rows are updated by K3)
    __device__ void finalize(double) const {}
};

// ---- K2: v~ <- P (J'u~ + d ux~)/beta - beta v ; publishes the block partials of sum(v~^2) -------
// norm(::DampenedVector) exactly as the reference writes it: sqrt(norm(y)^2 + norm(x)^2), iterative_lsmr.jl:72 -- the
// square of a square root is not the sum it came from, so this is NOT sqrt(sum y^2 + sum x^2) in the last bit.
__device__ __forceinline__ double dampened_norm(double sumsq_y, double sumsq_x) {
    const double ny = sqrt(sumsq_y), nx = sqrt(sumsq_x);
    return sqrt(ny * ny + nx * nx);
}

// beta = norm(u~) is formed by every block from K1's partials (lsmr.jl:119, il:72).
struct EpiV {
    static constexpr bool REDUCE = true;
    using defer = void;
    const int *done;
    int extra_blocks;
    LsmrState *st;
    const double *pu;   // K1's (or k_lsmr_begin's) partials of sum(u~_y^2)
    const int *npu;
    const double *px;   // K3's partials of sum(u~_x^2) (damped rows), or null
    const int *npx;
    const double *P;
    const double *dg;
    const double *ux;   // null during setup (zerosvector)
    double *v;
    double *partials;   // pv
    int *npartials;
    unsigned *counter;  // unused (deferred)
    double beta, inv_beta;
    int beta_zero, first;
    double *vout = nullptr;   // where v~ goes (null: in place, over v).  The three-launch iteration (lsq_lsmr3.h) keeps the
                              // normalised v and the new v~ apart: its next launch reads v~ while it rewrites v
    const double *cs = nullptr;   // ... and takes the gather vector of its next J*v straight from here: wout = (v~ .* P) .* s
    double *wout = nullptr;       // (s: the column scale of J = V diag(s), or null)
    // k_combine requests the column's own operands with its first round of partials (has_col_prefetch): seg() finds them in
    // registers when it is called for THAT column (the workgroup's first and, on the LSMR path, only column block)
    using has_col_prefetch = void;
    int pf_j = -1;
    double pf_P = 1.0, pf_dg = 0.0, pf_ux = 0.0, pf_v = 0.0, pf_cs = 1.0;
    __device__ void col_prefetch(int j) {
        pf_j = j;
        pf_P = P ? P[j] : 1.0;
        pf_dg = dg ? dg[j] : 0.0;
        pf_ux = (dg && ux) ? ux[j] : 0.0;
        pf_v = v[j];
        pf_cs = (wout && cs) ? cs[j] : 1.0;
    }
    using has_block_prepare = void;
    __device__ void block_prepare() {
        double b2, bx, unused;
        ordered_sum256x3(pu, npu, px, npx, nullptr, nullptr, b2, bx, unused);
        beta = dg ? dampened_norm(b2, px ? bx : 0.0) : sqrt(b2);   // (px null in the setup pass: u~x == 0)
        beta_zero = !(beta > 0.0);
        inv_beta = beta > 0.0 ? 1.0 / beta : 1.0;   // lsmr.jl:120-121 rmul!(u, inv(beta))
        first = st->first;
    }
    __device__ void seg(int j, double dot, double &racc) const {
        if (beta_zero) {                            // lsmr.jl:120: v (and alpha) stay as they are
            // The three-launch iteration reads v~ and the gather vector from buffers of their own and rescales them by 1/alpha:
            // with beta == 0 they must hold the NORMALISED v (the consumer's scale is 1 then, lsmr_scalars), not the previous
            // iteration's unnormalised v~.  Setup pass (first): v is still zero (lsmr.jl:76 never ran).
            if (vout) {
                const double vj = first ? 0.0 : v[j];
                vout[j] = vj;
                if (wout) {
                    const double t = P ? vj * P[j] : vj;
                    wout[j] = cs ? t * cs[j] : t;
                }
                racc += vj * vj;
            }
            return;
        }
        const bool pf = j == pf_j;                  // (the same operands, fetched a round trip earlier)
        double w = dot;
        if (dg && ux) w += (pf ? pf_ux : ux[j]) * (pf ? pf_dg : dg[j]);           // iterative_lsmr.jl:107
        w *= inv_beta;                              // u = u~/beta
        const double Pj = P ? (pf ? pf_P : P[j]) : 1.0;
        if (P) w *= Pj;                             // :41
        double vn = first ? w : w - beta * (pf ? pf_v : v[j]);    // :42-49 (beta == 0 => fill!)
        (vout ? vout : v)[j] = vn;
        if (wout) {
            const double t = P ? vn * Pj : vn;
            wout[j] = cs ? t * (pf ? pf_cs : cs[j]) : t;
        }
        racc += vn * vn;
    }
    __device__ void extra(int, double &) const {}
    __device__ void finalize(double) const {}
};

// alpha, beta and the rotations of one iteration on a private copy of the state (one thread)
__device__ __forceinline__ void lsmr_scalars(LsmrState &ns, double beta2, double betax2, double alpha2, bool damped, bool have_px) {
    const double beta = damped ? dampened_norm(beta2, have_px ? betax2 : 0.0) : sqrt(beta2);   // (no px in the setup pass)
    ns.beta = beta;
    ns.beta_zero = !(beta > 0.0);
    if (!ns.beta_zero) {
        ns.alpha = sqrt(alpha2);                       // lsmr.jl:77,123
        ns.vscale = ns.alpha > 0.0 ? 1.0 / ns.alpha : 1.0;
    } else {
        if (ns.first) ns.alpha = 0.0;
        ns.vscale = 1.0;                               // v was left untouched (lsmr.jl:120)
    }
    const double alpha = ns.alpha;
    if (ns.first) {                                    // lsmr.jl:82-113
        ns.zetabar = alpha * beta;
        ns.alphabar = alpha;
        ns.rho = 1.0; ns.rhobar = 1.0; ns.cbar = 1.0; ns.sbar = 0.0;
        ns.betadd = beta; ns.betad = 0.0; ns.rhodold = 1.0; ns.tautildeold = 0.0;
        ns.thetatilde = 0.0; ns.zeta = 0.0; ns.d = 0.0;
        ns.normA = -1.0; ns.condA = -1.0; ns.normx = -1.0;
        ns.normA2 = alpha * alpha;
        ns.maxrbar = 0.0; ns.minrbar = 1e100;
        ns.normb = beta; ns.normr = beta; ns.normAr = alpha * beta;
    } else {
        lsmr_rotate_inline(ns, alpha, beta);
    }
    ns.cu = beta > 0.0 ? alpha / beta : alpha;         // next K1: u~_new = A v - (alpha/beta) u~
}

// ||x||, the 7 stopping rules and the commit of the new state (one thread of the last block)
__device__ __forceinline__ void lsmr_commit(LsmrState &s, double total, LsmrState *st, LsqMailbox *mail) {
    if (s.first) {
        s.first = 0;
        if (!(s.normAr != 0.0)) { s.done = 1; s.notdone = 0; }      // lsmr.jl:115: exit if b = 0 or A'b = 0
        *st = s;
        publish(mail, st);
        return;
    }
    s.iter += 1;
    s.normx = sqrt(total);                       // lsmr.jl:206
    double test1 = s.normr / s.normb;
    double test2 = s.normAr / (s.normA * s.normr);
    double test3 = 1.0 / s.condA;
    double t1 = test1 / (1.0 + s.normA * s.normx / s.normb);
    double rtol = s.btol + s.atol * s.normA * s.normx / s.normb;
    int istop = 0;                               // :224-231, first hit wins
    if (s.iter >= s.maxiter) istop = 7;
    else if (1.0 + test3 <= 1.0) istop = 6;
    else if (1.0 + test2 <= 1.0) istop = 5;
    else if (1.0 + t1 <= 1.0) istop = 4;
    else if (test3 <= s.ctol) istop = 3;
    else if (test2 <= s.atol) istop = 2;
    else if (test1 <= rtol) istop = 1;
    s.istop = istop;
    if (istop) { s.done = 1; s.notdone = 0; }
    *st = s;
    // (hints for the host's prediction of the stop iteration: in front of the word that announces the iteration)
    __hip_atomic_store((double *)&mail->test1, test1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store((double *)&mail->test2, test2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    publish(mail, st);
}

// ---- K3: alpha, rotations (every block, redundantly and identically), n-vector updates, ||x||,
//          stopping rules and the commit of the new state (last block) --------------------------
__global__ void __launch_bounds__(LSQ_NT)
k_lsmr_update(int n, LsmrState *st, LsqMailbox *mail, const double *pu, const int *npu, const double *pv,
              const int *npv, const double *px_in, const int *npx_in, double *px, int *npx,
              const double *__restrict__ dg, double *__restrict__ ux,
              const double *__restrict__ P, double *__restrict__ v, double *__restrict__ h,
              double *__restrict__ hbar, double *__restrict__ x, double *__restrict__ xout,
              double *__restrict__ t, double *partials, unsigned *counter) {
    __shared__ double sh[LSQ_NT / 64];
    __shared__ LsmrState ns;   // this iteration's state, computed from the committed one
    // This kernel is a chain of memory latencies (it moves 0.5 MB): everything that does not depend on the scalars is
    // fetched up front, together -- the thread's vector elements, the committed state (one coalesced load into LDS; it
    // also carries the `done` flag of a finished solve) and, inside ordered_sum256x3, counts and partials -- so that one
    // round trip is paid instead of five.
    const int tid = threadIdx.x;
    const int j0 = blockIdx.x * LSQ_NT + tid, jc = j0 < n ? j0 : n - 1;
    const double e_v = v[jc], e_h = h[jc], e_hb = hbar[jc], e_x = x[jc];
    const double e_P = P ? P[jc] : 1.0, e_dg = dg ? dg[jc] : 0.0, e_ux = dg ? ux[jc] : 0.0;
    static_assert(sizeof(LsmrState) % 8 == 0 && sizeof(LsmrState) / 8 <= LSQ_NT, "state copy: one 8-byte word per thread");
    if (tid < (int)(sizeof(LsmrState) / 8)) ((unsigned long long *)&ns)[tid] = ((const unsigned long long *)st)[tid];
    double beta2, betax2, alpha2;
    ordered_sum256x3(pu, npu, px_in, npx_in, pv, npv, beta2, betax2, alpha2);   // (its barriers also publish ns)
    if (ns.done) return;
    if (threadIdx.x == 0) lsmr_scalars(ns, beta2, betax2, alpha2, dg != nullptr, px_in != nullptr);
    __syncthreads();
    const bool first = ns.first;
    const double vs = ns.vscale, c1 = ns.c1, c2 = ns.c2, c3 = ns.c3, cu = ns.cu;
    double acc = 0.0, accx = 0.0;
    for (int j = j0; j < n; j += gridDim.x * LSQ_NT) {
        const bool pf = j == j0;                     // first trip: the prefetched elements
        const double Pj = P ? (pf ? e_P : P[j]) : 1.0;
        double vj = (pf ? e_v : v[j]) * vs;          // lsmr.jl:78,124 rmul!(v, inv(alpha))
        v[j] = vj;
        if (first) {                                 // :89-90, iterative_lsmr.jl:183,242
            h[j] = vj;
            hbar[j] = 0.0;
            x[j] = 0.0;
            xout[j] = 0.0;
        } else {
            const double hj = pf ? e_h : h[j];
            double hb = (pf ? e_hb : hbar[j]) * c1 + hj;   // :152-153
            hbar[j] = hb;
            double xj = (pf ? e_x : x[j]) + c2 * hb;       // :154
            x[j] = xj;
            h[j] = hj * c3 + vj;                     // :155-156
            acc += xj * xj;
            // the caller's x always holds P.*x of the newest iterate (iterative_lsmr.jl:195-196,
            // 256-257), so no launch is needed once the stopping rule fires
            xout[j] = P ? xj * Pj : xj;
        }
        const double tj = P ? vj * Pj : vj;          // iterative_lsmr.jl:31 ldiv!(tmp, P, a)
        t[j] = tj;
        if (dg) {   // damped rows of the NEXT u (iterative_lsmr.jl:92): u~x <- d.*t - cu*u~x
            double un = tj * (pf ? e_dg : dg[j]) - cu * (pf ? e_ux : ux[j]);
            ux[j] = un;
            accx += un * un;
        }
    }
    if (dg) {       // deferred partials of sum(u~x^2): read by the next K2 / K3
        double bx = block_sum<LSQ_NT>(accx, sh);
        if (threadIdx.x == 0) {
            px[blockIdx.x] = bx;
            if (blockIdx.x == 0) *npx = (int)gridDim.x;
        }
    }
    double bv = block_sum<LSQ_NT>(acc, sh);
    // last block: every other block is past its prologue, so the state can be committed
    grid_reduce<LSQ_NT>(bv, partials, counter, gridDim.x, sh, [&](double total) { lsmr_commit(ns, total, st, mail); });
}

// (Measured and dropped in round 2: K2's two passes + K3 as ONE launch for the sliced columns, one resident workgroup per CU
//  with two grid barriers -- hierarchical tickets + a polled flag, ~2.2 us each -- and v~ kept in registers.  42.7 us against
//  25.3 + 5.9 + 9.0 us in three launches: the barriers cost what the two launch ramps cost; 2885 vs 2874-2895 LM it/s on C4.)

#include "lsq_lsmr3.h"

// ---- setup from the caller's J'y in one launch: P, sqrt(damp), state reset and
// v~ = P.*(J'y)/beta_1 with the block partials of sum(v~^2)  (k_lsmr_prep + k_lsmr_begin +
// k_combine<EpiV> of the general path; k_lsmr_update in "first" mode follows).
// beta_1^2 = sum(y^2) comes from the caller when it already holds it (the LM loop's ssr), else
// from k_lsmr_begin's partials.
__global__ void __launch_bounds__(LSQ_NT)
k_lsmr_setup(int n, const double *__restrict__ colsum, double *__restrict__ damp, double *__restrict__ P,
             double *__restrict__ dg, double *__restrict__ ux, const double *__restrict__ Jty,
             double *__restrict__ v, LsmrState *st, double *pu, int *npu, double ysumsq, double *pv, int *npv,
             double atol, double btol, double ctol, int maxiter, unsigned epoch, int custom_p,
             const double *__restrict__ cs = nullptr, double *__restrict__ wout = nullptr) {
    __shared__ double sh[LSQ_NT / 64];
    const double beta2 = ysumsq >= 0.0 ? ysumsq : ordered_sum256(pu, *npu);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->iter = 0; st->istop = 0; st->done = 0; st->notdone = 1; st->first = 1;
        st->atol = atol; st->btol = btol; st->ctol = ctol;
        st->maxiter = maxiter; st->epoch = epoch; st->cu = 0.0;
        if (ysumsq >= 0.0) {
            pu[0] = ysumsq;
            *npu = 1;
        }
    }
    const double beta = damp ? dampened_norm(beta2, 0.0) : sqrt(beta2);   // u_x = 0 (zerosvector, il:246)
    const bool beta_zero = !(beta > 0.0);
    const double inv_beta = beta > 0.0 ? 1.0 / beta : 1.0;
    double acc = 0.0;
    for (int j = blockIdx.x * LSQ_NT + threadIdx.x; j < n; j += gridDim.x * LSQ_NT) {
        double s = colsum[j];
        if (damp) {
            double d = damp[j];
            s += d;                  // iterative_lsmr.jl:251
            double r = sqrt(d);      // :252
            dg[j] = r;
            damp[j] = r;
            ux[j] = 0.0;             // zerosvector (:246)
        }
        const double Pj = custom_p ? P[j] : (s > 0.0 ? 1.0 / sqrt(s) : 0.0);
        P[j] = Pj;
        if (!beta_zero) {            // lsmr.jl:76 (beta == 0: v is left untouched, :120)
            const double w = Jty[j] * inv_beta * Pj;
            v[j] = w;
            if (wout) wout[j] = cs ? (w * Pj) * cs[j] : w * Pj;     // the gather vector of the first J*v (lsq_lsmr3.h)
            acc += w * w;
        }
    }
    double bv = block_sum<LSQ_NT>(acc, sh);
    if (threadIdx.x == 0) {
        pv[blockIdx.x] = bv;
        if (blockIdx.x == 0) *npv = (int)gridDim.x;
    }
}

// ---- LM + LSMR, n <= LSMR_LM_PREP_MAX_N: the LM loop's damping + projected gradient norm (k_lm_damp_grad,
// levenberg_marquardt.jl:82-86, 102-104) and k_lsmr_setup as ONE launch of 1024-thread workgroups.  The damping needs
// mean(colsum) -- a reduction over all n -- before the first element can be written: every workgroup takes it itself, over
// all n, in exactly the order of the one-workgroup kernel it replaces (thread-sequential with stride 1024, wave tree, 16
// waves in order: same bits), then handles its own 1024 elements.  One n-length launch (~6 us of latency) less per outer
// iteration; sum(v~^2) is taken per 1024 elements instead of per 256.
__global__ void __launch_bounds__(1024)
k_lm_lsmr_setup(int n, LsmrLmPrep lm, double *__restrict__ damp, double *__restrict__ P, double *__restrict__ dg,
                double *__restrict__ ux, const double *__restrict__ g, double *__restrict__ v, LsmrState *st, double *pu, int *npu,
                double ysumsq, double *pv, int *npv, double atol, double btol, double ctol, int maxiter, unsigned epoch,
                const double *__restrict__ colscale = nullptr, double *__restrict__ wout = nullptr) {
    constexpr int R = LSMR_LM_PREP_MAX_N / 1024;
    __shared__ double sh[16], shm[16];
    __shared__ double s_mean;
    const int tid = threadIdx.x;
    double cs[R], gv[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {   // every load is issued before the first use
        const int i = tid + k * 1024;
        cs[k] = i < n ? lm.colsum[i] : 0.0;
        gv[k] = i < n ? g[i] : 0.0;
    }
    double acc = 0.0, mg = 0.0;
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int i = tid + k * 1024;
        if (i < n) {
            acc += cs[k];
            double gi = gv[k];
            if (lm.lo && lm.x[i] <= lm.lo[i] && gi > 0.0) gi = 0.0;
            else if (lm.hi && lm.x[i] >= lm.hi[i] && gi < 0.0) gi = 0.0;
            double a = fabs(gi);
            if (isnan(a)) a = INFINITY;
            mg = fmax(mg, a);
        }
    }
    acc = wave_sum(acc);
    mg = wave_max(mg);
    if ((tid & 63) == 0) {
        sh[tid >> 6] = acc;
        shm[tid >> 6] = mg;
    }
    __syncthreads();
    if (tid == 0) {
        double tt = 0.0, tm = shm[0];
        for (int w = 0; w < 16; ++w) tt += sh[w];
        for (int w = 1; w < 16; ++w) tm = fmax(tm, shm[w]);
        s_mean = tt / n;
        if (blockIdx.x == 0) {
            *lm.out_grad = tm;
            st->iter = 0; st->istop = 0; st->done = 0; st->notdone = 1; st->first = 1;
            st->atol = atol; st->btol = btol; st->ctol = ctol;
            st->maxiter = maxiter; st->epoch = epoch; st->cu = 0.0;
            pu[0] = ysumsq;
            *npu = 1;
        }
    }
    __syncthreads();
    const double lo_d = lm.min_diag * s_mean, hi_d = lm.max_diag * s_mean;
    const double beta = dampened_norm(ysumsq, 0.0);   // u_x = 0 (zerosvector, il:246)
    const bool beta_zero = !(beta > 0.0);
    const double inv_beta = beta > 0.0 ? 1.0 / beta : 1.0;
    double a2 = 0.0;
    const int j = blockIdx.x * 1024 + tid;             // (this workgroup's own elements: blockIdx.x-th group of 1024)
    if (j < n) {
        // the values of element j sit in this thread's registers when blockIdx.x < R: cs / gv are indexed by a constant after
        // unrolling, so pick by selection
        double c0 = 0.0, g0 = 0.0;
#pragma unroll
        for (int k = 0; k < R; ++k)
            if (k == (int)blockIdx.x) { c0 = cs[k]; g0 = gv[k]; }
        double c = c0;
        c = c > hi_d ? hi_d : (c < lo_d ? lo_d : c);
        const double d = c * lm.inv_delta;     // rmul!(dtd, 1/Delta)
        const double s = c0 + d;               // iterative_lsmr.jl:251
        const double r = sqrt(d);              // :252
        dg[j] = r;
        damp[j] = r;
        ux[j] = 0.0;                           // zerosvector (:246)
        const double Pj = s > 0.0 ? 1.0 / sqrt(s) : 0.0;
        P[j] = Pj;
        if (!beta_zero) {                      // lsmr.jl:76 (beta == 0: v is left untouched, :120)
            const double w = g0 * inv_beta * Pj;
            v[j] = w;
            if (wout) wout[j] = colscale ? (w * Pj) * colscale[j] : w * Pj;     // the gather vector of the first J*v (lsq_lsmr3.h)
            a2 = w * w;
        }
    }
    __syncthreads();
    const double bv = block_sum<1024>(a2, sh);
    if (tid == 0) {
        pv[blockIdx.x] = bv;
        if (blockIdx.x == 0) *npv = (int)gridDim.x;
    }
}

// ---- row-sharded adjoint product: buf[0..n) = J_p'u_p, buf[n] = sum(u_p.^2) -> all-reduce -> epilogue ----
struct EpiBuf {   // out[j] = dot
    static constexpr bool REDUCE = false;
    const int *done;
    int extra_blocks;
    double *out;
    double *partials;
    unsigned *counter;
    __device__ void seg(int j, double dot, double &) const { out[j] = dot; }
    __device__ void extra(int, double &) const {}
    __device__ void finalize(double) const {}
};
__global__ void __launch_bounds__(LSQ_NT) k_rowshard_sumsq(const double *pu, const int *npu, double *out, const int *done,
                                                            double *xbuf, int n) {
    if (done && *done) {
        // an iteration queued behind the stop (the rest of a look-ahead chunk): its product returned at once and the buffer still
        // holds the LAST all-reduced vector, which the coming collective would sum again (x world per queued iteration, for
        // nobody to read -- but it must not run off to Inf): clear it
        for (int i = threadIdx.x; i <= n; i += LSQ_NT) xbuf[i] = 0.0;
        return;
    }
    double a, b, c2;
    ordered_sum256x3(pu, npu, nullptr, nullptr, nullptr, nullptr, a, b, c2);
    if (threadIdx.x == 0) *out = a;
}
extern "C" int lsq_solver_set_row_allreduce(lsq_solver *s, lsq_device_allreduce_callback cb, void *user, long long global_rows) {
    if (!s || s->kind != LSQ_LSMR) {
        lsq_set_error("row-sharded solves: LSMR() only");
        return LSQ_EARG;
    }
    s->row_cb = cb;
    s->row_user = user;
    s->global_rows = cb ? global_rows : 0;
    s->colsum_g_uid = 0;                // (another hook = another group of ranks: the summed colsumabs2 is theirs, not ours)
    s->colsum_g_version = ~0ull;
    if (cb && !s->d_xbuf) {
        // (n + 1 doubles travel; the slot behind them is read as a partial-sum array of count 1, and ordered_sum256x3
        //  fetches the first 256 entries of such an array before it looks at the count)
        LSQ_HIP(hipMalloc(&s->d_xbuf, (size_t)(s->n + 2 + 256) * sizeof(double)));
        LSQ_ZERO(s->d_xbuf, 0, (size_t)(s->n + 2 + 256) * sizeof(double));
        LSQ_HIP(hipMalloc(&s->d_one, sizeof(int)));
        const int one = 1;
        LSQ_HIP(hipMemcpy(s->d_one, &one, sizeof(int), hipMemcpyHostToDevice));
    }
    return LSQ_OK;
}
// colsumabs2 of the whole Jacobian for a row-sharded solver (lsq_solver.h: d_colsum_g): one collective per Jacobian version,
// issued by every rank at the same point of its call sequence; unsharded solvers get the handle's cache
int lsq_rowshard_colsum(lsq_solver *s, lsq_mat *J, const double **out) {
    const double *local = lsq_cached_colsum(J);
    if (!local) return LSQ_EHIP;
    *out = local;
    if (!s->row_cb) return LSQ_OK;
    lsq_ctx *c = s->ctx;
    if (!s->d_colsum_g) LSQ_HIP(hipMalloc(&s->d_colsum_g, (size_t)(s->n > 0 ? s->n : 1) * sizeof(double)));
    if (s->colsum_g_uid != J->uid || s->colsum_g_version != J->version) {
        LSQ_TRY(lsq_d2d(c, s->d_colsum_g, local, (size_t)J->n * sizeof(double)));   // (a copy kernel: no runtime-side staging hole)
        if (s->row_cb(s->d_colsum_g, J->n, (void *)c->stream, s->row_user) != 0) {
            lsq_set_error("row all-reduce callback reported failure");
            return LSQ_ECALLBACK;
        }
        s->colsum_g_uid = J->uid;
        s->colsum_g_version = J->version;
    }
    *out = s->d_colsum_g;
    return LSQ_OK;
}
// v~ <- epilogue(sum over ranks of J_p'src_p) with beta from the summed sum(src.^2); `ev` is the unsharded epilogue
static int rowshard_adjoint(lsq_solver *s, lsq_mat *J, const double *src, EpiV ev, const double *pu, const int *npu) {
    lsq_ctx *c = s->ctx;
    const int n = J->n;
    EpiBuf eb{ev.done, 0, s->d_xbuf, nullptr, nullptr};
    LSQ_TRY(launch_product(J, 1, src, eb));
    LSQ_LAUNCH(k_rowshard_sumsq, dim3(1), dim3(LSQ_NT), 0, c->stream, pu, npu, s->d_xbuf + n, ev.done, s->d_xbuf, n);
    LSQ_HIP(hipGetLastError());
    if (s->row_cb(s->d_xbuf, n + 1, (void *)c->stream, s->row_user) != 0) {
        lsq_set_error("row all-reduce callback reported failure");
        return LSQ_ECALLBACK;
    }
    ev.pu = s->d_xbuf + n;
    ev.npu = s->d_one;
    const int nb = lsq_div_up(n, LSQ_CMB_COLS);
    LSQ_LAUNCH((k_combine<EpiV>), dim3(std::min(nb, 2048)), dim3(LSQ_NT), 0, c->stream, s->d_xbuf, n, 1, ev, nb);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

int lsq_lsmr_alloc(lsq_solver *s) {
    size_t nb = (size_t)(s->n > 0 ? s->n : 1) * sizeof(double);
    LSQ_HIP(hipMalloc(&s->d_state, 2 * sizeof(LsmrState)));    // (two: the three-launch iteration double-buffers it)
    LSQ_ZERO(s->d_state, 0, 2 * sizeof(LsmrState));
    // the three-launch iteration (lsq_lsmr3.h): second copies of x, hbar, h; sum(u~^2) partials x 2; the three norms x 2; counts
    s->f3_elems = 4 * (size_t)(s->n > 0 ? s->n : 1) + 2 * 4096 + 8 + 16 + 8;
    LSQ_HIP(hipMalloc(&s->d_f3, s->f3_elems * sizeof(double)));
    LSQ_ZERO(s->d_f3, 0, s->f3_elems * sizeof(double));
    LSQ_HIP(hipMalloc(&s->d_u, (size_t)(s->m > 0 ? s->m : 1) * sizeof(double)));
    LSQ_HIP(hipMalloc(&s->d_ux, nb));
    LSQ_HIP(hipMalloc(&s->d_v, nb));
    LSQ_HIP(hipMalloc(&s->d_h, nb));
    LSQ_HIP(hipMalloc(&s->d_hbar, nb));
    LSQ_HIP(hipMalloc(&s->d_t, nb));
    LSQ_HIP(hipMalloc(&s->d_P, nb));
    LSQ_HIP(hipMalloc(&s->d_dg, nb));
    LSQ_HIP(hipMalloc(&s->d_rhs, nb));  // LSMR iterate (un-preconditioned space)
    LSQ_HIP(hipMalloc(&s->d_red, 4 * 4096 * sizeof(double) + 64));  // pu, pv, px[2] (4096 each), counts
    LSQ_ZERO(s->d_red, 0, 4 * 4096 * sizeof(double) + 64);
    return LSQ_OK;
}

void lsq_lsmr_free(lsq_solver *s) {
    hipFree(s->d_state); hipFree(s->d_u); hipFree(s->d_ux); hipFree(s->d_v); hipFree(s->d_h);
    hipFree(s->d_hbar); hipFree(s->d_t); hipFree(s->d_P); hipFree(s->d_dg); hipFree(s->d_rhs); hipFree(s->d_red);
    hipFree(s->d_xbuf); hipFree(s->d_one); hipFree(s->d_colsum_g); hipFree(s->d_f3);
}

static inline int nvec_grid(const lsq_ctx *c, int n) {
    int g = lsq_div_up(n > 0 ? n : 1, LSQ_NT);
    int cap = c->num_cus * 4;
    return g > cap ? cap : g;
}

// d_damp == nullptr: undamped (Dogleg, atol = btol = 1e-6); else LM (btol = 0.5).
bool lsq_lsmr_takes_lm_prep(const lsq_solver *s, const lsq_mat *J) {
    // (row-sharded: every rank must take the same kernels -- their summation orders differ in the last bits, and ranks whose
    //  replicated scalars differ stop at different inner iterations, i.e. issue different numbers of collectives; so the choice
    //  may depend on n only, never on the size of this rank's row block)
    return s->kind == LSQ_LSMR && J->n <= LSMR_LM_PREP_MAX_N && (s->row_cb || !lsq_small_mat(J)) && !s->precond_cb && !s->gen_ldiv &&
           !getenv("LSQ_LSMR_SEPARATE_SETUP");
}

// ---- the host side of a solve: what the two loops below share -----------------------------------------------------------------
// the progress word as the host reads it (layout: publish)
struct LsmrProgress {
    bool ours, done;     // written by THIS solve (its epoch) / that solve is over
    int istop, iter;
    LsmrProgress(unsigned long long w, unsigned epoch)
        : ours((unsigned)(w >> 41) == epoch), done(((w >> 40) & 1ull) != 0), istop((int)((w >> 32) & 0xff)), iter((int)(w & 0xffffffffu)) {}
};
static inline unsigned long long lsmr_progress_word(const lsq_ctx *c) { return *(volatile unsigned long long *)c->h_mail; }

// Where the solve will stop, predicted from the hints the device publishes beside the progress word: test1 = |r|/|b| and
// test2 = |A'r|/(|A||r|).  A solve is over when test1 <= btol (+ a 1e-6-sized term) or test2 <= atol (lsmr.jl:224-231; the other
// rules do not fire on these operators), and on the damped, Jacobi-preconditioned operators of an LM run test2 falls
// geometrically (C4: x 0.07-0.09 per iteration, every iteration).
struct StopPredictor {
    double t1_prev, t2_prev, ratio2;   // (-1: none yet); ratio2 = test2(k) / test2(k-1), at first the previous solve's (lsq_solver::lsmr_ratio2)
    int hint_it;                       // last iteration whose hints went into the prediction
    // `w`: the progress word that announced iteration `it`.  Returns the planned last iteration, or 0 (nothing new to say).
    int update(const LsqMailbox *mail, unsigned long long w, int it, double atol, double btol) {
        if (!(it > hint_it && it >= 1)) return 0;
        const double h1 = mail->test1, h2 = mail->test2;
        const unsigned long long w2 = *(volatile unsigned long long *)mail;
        if (!(w2 == w && h1 > 0.0 && h2 > 0.0)) return 0;   // (the pair belongs to iteration `it` only if the word did not move meanwhile)
        if (t2_prev > 0.0 && h2 < t2_prev) ratio2 = std::min(0.95, std::max(1e-4, h2 / t2_prev));
        int k = 1 << 20;
        if (h2 > atol && ratio2 < 1.0) k = std::min(k, (int)std::ceil(std::log(atol / h2) / std::log(ratio2) - 1e-9));
        if (t1_prev > 0.0 && h1 < 0.98 * t1_prev && h1 > btol)       // test1 still falling: when does it reach btol?
            k = std::min(k, (int)std::ceil(std::log(btol / h1) / std::log(h1 / t1_prev) - 1e-9));
        t1_prev = h1; t2_prev = h2; hint_it = it;
        return k < (1 << 20) ? it + std::max(1, k) : 0;
    }
};

struct LsmrRun {     // what a loop knows about its solve
    int it = 0, istop = 0;
    bool finished = false;
    bool tail_ran = false;      // a guarded tail, queued inside the loop, is known to have run
    bool see(const LsmrProgress &p) {     // true: the solve is over
        if (p.ours) it = p.iter;
        if (p.ours && p.done) { istop = p.istop; finished = true; }
        return finished;
    }
};

// The waiting host's fallback (every 1024th idle poll).  A failed stream will never move the mailbox: error.  A drained stream
// whose progress word is neither final nor at `committed` (the iteration the newest enqueued launch commits) means the mailbox
// is not visible (should not happen with coherent host memory): read the state `d_st` instead.  `spent`: the iteration budget
// is used up, i.e. nothing more will be enqueued.
static int lsmr_stream_drained(lsq_ctx *c, unsigned epoch, int committed, const LsmrState *d_st, bool spent, LsmrRun &r) {
    const hipError_t sq = hipStreamQuery(c->stream);
    if (sq != hipSuccess && sq != hipErrorNotReady) {   // launch failure / device fault
        lsq_set_error("HIP error inside the LSMR iteration: %s", hipGetErrorString(sq));
        return LSQ_EHIP;
    }
    if (sq != hipSuccess) return LSQ_OK;
    // stream drained: whatever the mailbox shows now is final for the enqueued work
    const LsmrProgress p(lsmr_progress_word(c), epoch);
    if (p.ours && (p.done || p.iter >= committed)) return LSQ_OK;    // (the loop reads it next)
    LsmrState hs;
    LSQ_HIP(hipMemcpy(&hs, d_st, sizeof(hs), hipMemcpyDeviceToHost));
    r.it = hs.iter;
    if (hs.done) {
        r.istop = hs.istop;
        r.finished = true;
    } else if (spent) {
        lsq_set_error("lsmr: iteration budget exhausted without a stop rule");
        return LSQ_EHIP;
    }
    return LSQ_OK;
}

// instrumentation: launches queued beyond the stopping iteration returned on their first instruction (the K1' that committed the
// stop skipped its product) -- drop their samples so the reported average is over working launches only
struct LsmrProf {
    size_t base[2];                // samples per kernel id that were there before this solve
    std::vector<int> iter[2];      // iteration number (1-based) of every timed launch of this solve
};
static void lsmr_drop_idle_samples(lsq_ctx *c, LsmrProf &p, int it) {
    for (int k = 0; k < 2; ++k) {
        auto &v = c->prof_ev[k];
        while (v.size() > p.base[k] && !p.iter[k].empty() && p.iter[k].back() > it) {
            hipEventDestroy(v.back()); v.pop_back();
            hipEventDestroy(v.back()); v.pop_back();
            p.iter[k].pop_back();
        }
    }
}

// One solve's operands, constants and its view of the solver's buffers, built once by lsq_lsmr_solve
struct LsmrWork {
    lsq_solver *s;
    lsq_ctx *c;
    lsq_mat *J;
    const double *d_y;
    double *d_x;
    int m, n;
    bool damped, sharded;
    bool fused;                    // the three-launch iteration (lsq_lsmr3.h); else K1 | K2 | K3
    double atol, btol, conlim;
    int maxiter, lookahead;
    unsigned epoch;
    int gn;                        // grid of the n-vector kernels
    const double *dgk;             // sqrt(damp), or null
    const LsmrTail *tail;          // the caller's (may be null)
    bool dynamic, spec;            // the stop is predicted from the solve's own hints / the tail's place depends on a guess at all
    LsmrState *stb[2];             // the three-launch iteration double-buffers the state; the four-launch one lives in [0]
    double *pu, *pv;               // deferred-reduction partials (sum u~^2 / sum v~^2); fused: pu is fpu[0]
    int *npu, *npv;
    double *pxb[2];                // sum(u~x^2) partials, double-buffered: K3 reads iteration k's while writing k+1's
    int *npxb[2];
    double *vset;                  // where the setup (and every K2) leaves v~
    // the three-launch iteration's second copies (lsq_lsmr_alloc: d_f3)
    double *fx[2], *fhbar[2], *fh[2];
    double *fw;                    // gather vector of the next J*v: (v~ .* P) .* s
    double *fpu[2];
    int *fnpu;                     // two counts
    LsmrHandoff *fho;              // the in-launch record of k_lsmr_fused
};

// K2's epilogue on the four-launch loop's buffers, as the setup uses it (no u~x, no px yet)
static EpiV lsmr_epi_v(const LsmrWork &W) {
    return EpiV{&W.stb[0]->done, 0, W.stb[0], W.pu, W.npu, nullptr, nullptr, W.s->d_P, W.dgk, nullptr, W.s->d_v, W.pv, W.npv,
                nullptr, 0.0, 0.0, 0, 0};
}
// K3 of the four-launch loop.  px_in: the partials of this iteration's sum(u~x^2) (null in the setup: u~x is still zero, so only
// sum(u~_y^2) enters beta_1), `out`: the px buffer that receives the next iteration's.  `summed`: sum(u~_y^2) is the ranks' sum
// that rowshard_adjoint left behind the all-reduced vector, not this rank's partials
static void lsmr_launch_update(const LsmrWork &W, bool summed, const double *px_in, const int *npx_in, int out) {
    lsq_solver *s = W.s; lsq_ctx *c = W.c;
    LSQ_LAUNCH(k_lsmr_update, dim3(W.gn), dim3(LSQ_NT), 0, c->stream, W.n, W.stb[0], c->d_mail,
                       summed ? (const double *)(s->d_xbuf + W.n) : (const double *)W.pu,
                       summed ? (const int *)s->d_one : (const int *)W.npu, W.pv, W.npv, px_in, npx_in, W.pxb[out], W.npxb[out],
                       W.dgk, s->d_ux, s->d_P, s->d_v, s->d_h, s->d_hbar, s->d_rhs, W.d_x, s->d_t, c->d_partials, lsq_ctr(c, 3));
}

// P, sqrt(damp), the state reset and v~ = P.*(A'b)/beta_1; the four-launch loop's K3 in "first" mode behind it (the three-launch
// iteration's first K1' does that itself)
static int lsmr_enqueue_setup(const LsmrWork &W, double *d_damp, const double *d_Jty, double y_sumsq, const LsmrLmPrep *lm,
                              const double *colsum, int custom_p) {
    lsq_solver *s = W.s; lsq_ctx *c = W.c; lsq_mat *J = W.J;
    const int m = W.m, n = W.n;
    LsmrState *st = W.stb[0];
    const double *cscale = W.fused ? J->d_colscale : nullptr;
    double *wout = W.fused ? W.fw : nullptr;
    bool summed = false;           // (a caller's J'y comes with sum(y^2) of ALL rows, or with every rank's own k_lsmr_begin)
    auto launch_begin = [&]() {
        long long gb = std::min<long long>(lsq_div_up(m > 0 ? m : 1, LSQ_NT), (long long)c->num_cus * 8);
        if (gb > 4096) gb = 4096;
        LSQ_LAUNCH(k_lsmr_begin, dim3((int)gb), dim3(LSQ_NT), 0, c->stream, m, W.d_y, st, W.pu, W.npu, W.atol,
                           W.btol, 1.0 / W.conlim, W.maxiter, W.epoch);
    };
    if (lm) {
        if (!(d_Jty && y_sumsq >= 0.0 && W.damped && lsq_lsmr_takes_lm_prep(s, J))) {
            lsq_set_error("lsmr: LM preparation requested where it does not apply");
            return LSQ_EARG;
        }
        LSQ_LAUNCH(k_lm_lsmr_setup, dim3(lsq_div_up(n, 1024)), dim3(1024), 0, c->stream, n, *lm, d_damp, s->d_P, s->d_dg,
                           s->d_ux, d_Jty, W.vset, st, W.pu, W.npu, y_sumsq, W.pv, W.npv, W.atol, W.btol, 1.0 / W.conlim, W.maxiter,
                           W.epoch, cscale, wout);
    } else if (d_Jty) {
        if (!(y_sumsq >= 0.0)) launch_begin();
        LSQ_LAUNCH(k_lsmr_setup, dim3(W.gn), dim3(LSQ_NT), 0, c->stream, n, colsum, d_damp, s->d_P, s->d_dg,
                           s->d_ux, d_Jty, W.vset, st, W.pu, W.npu, y_sumsq >= 0.0 ? y_sumsq : -1.0, W.pv, W.npv, W.atol, W.btol,
                           1.0 / W.conlim, W.maxiter, W.epoch, custom_p, cscale, wout);
    } else {
        LSQ_LAUNCH(k_lsmr_prep, dim3(W.gn), dim3(LSQ_NT), 0, c->stream, n, colsum, d_damp, s->d_P,
                           s->d_dg, s->d_ux, custom_p);
        launch_begin();
        LSQ_HIP(hipGetLastError());
        // v~ = A'u (setup)
        EpiV ev = lsmr_epi_v(W);
        if (W.fused) { ev.vout = W.vset; ev.cs = J->d_colscale; ev.wout = W.fw; }
        if (W.sharded) LSQ_TRY(rowshard_adjoint(s, J, W.d_y, ev, W.pu, W.npu));
        else LSQ_TRY(launch_product(J, 1, W.d_y, ev));
        summed = W.sharded;
    }
    if (!W.fused) lsmr_launch_update(W, summed, nullptr, nullptr, 0);     // it already forms iteration 1's u~x
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

// ---- three launches per inner iteration: K1' (k_lsmr_fused: decides iteration j-1, updates the n-vectors, J*v of iteration j) |
// K2a (k_sell_cols) | K2b (k_combine<EpiV>).  Launch j of K1' reads state / partials / x, hbar, h number (j-1)&1 and writes number
// j&1; it reports iteration j-1 in the progress word.
// The caller's tail: the host REACTS, it does not pre-place (round 6; profiles/r06/ab_tail_react.txt).  A guarded tail queued
// behind the launch that is expected to commit the stop costs nothing when the guess holds, but ~50 us when it does not: five
// launches of full grids that skip themselves stand between the solve's next product and the queue's head (measured: perfect
// first guesses would gain 3.6 % on C4).  Here the expected stop only makes that launch CAUTIOUS, and nothing more is queued
// until it has reported (~8 us into it): if the solve is over the caller (lsq_lsmr_solve) queues the tail, unguarded, while the
// cautious launch winds down; if not, the product of that launch is still streaming for 20 us and the next launches are queued
// behind it as usual.  A wrong guess then costs a late product.
// With the caller's step in hand (LsmrTail::step: the LM loop) that launch is k_lsmr_commit_step instead (lsq_lsmr3.h): ten
// workgroups on C4, no product workgroups that stage w only to find `done`, and on a stop the step is taken inside it -- no
// boundary, no k_step.  A wrong guess then costs that narrow launch and a host reaction in front of an ordinary launch.
static int lsmr_run_fused(const LsmrWork &W, StopPredictor &pred, LsmrRun &r) {
    lsq_solver *s = W.s; lsq_ctx *c = W.c; lsq_mat *J = W.J;
    const LsmrTail *tail = W.tail;
    const int m = W.m, n = W.n;
    int planned = W.spec ? tail->predict : 0;      // the iteration expected to be the last: the caller's guess, then the solve's own
    int wait_at = 0;             // the iteration whose commit (by a cautious launch) is awaited before anything else is queued
    bool wait_is_guess = false;  //   ... and that launch was cautious because of a PREDICTION (counted), not only because nothing was known
    const LsqSell &S = J->srows;
    const int nxpad = (n + 1) & ~1;
    const size_t lds = (size_t)(nxpad + LSQ_SELL_ROWS_MAX) * sizeof(double);
    LSQ_TRY(lsq_set_lds(c, (const void *)k_lsmr_fused<0>, (LSQ_LDS_X_MAX + LSQ_SELL_ROWS_MAX) * sizeof(double)));
    // update workgroups: the CUs the sliced rows leave without a block (C4: 253 blocks on 256 CUs -> 3), at least 3
    int ub = c->num_cus - S.nblocks;
    ub = ub < 3 ? 3 : (ub > LSQ_FUSED_UB_MAX ? LSQ_FUSED_UB_MAX : ub);
    const int pb = std::max(1, std::min(S.nblocks, c->num_cus - ub));
    int k1 = 0, enq = 0;         // K1' launches / whole iterations enqueued: k1 is enq or enq + 1
    const int test_no_record = getenv("LSQ_TEST_EXCHANGE_TIMEOUT") ? 1 : 0;       // (read once per solve, not per launch)
    // The caller handed over its step: where a cautious launch would go, k_lsmr_commit_step decides iteration k1 instead -- and
    // takes the step if the solve is over.  It is not a K1' launch: if it reports "not done" it has written nothing, and the
    // ordinary launch k1 + 1 is queued as if it had never run (plain_j: never a second commit launch for the same iteration).
    const bool commit_ok = W.spec && tail->step && tail->step_taken && !getenv("LSQ_NO_COMMIT_STEP");
    bool commit_pending = false; // a commit launch is deciding iteration wait_at
    int plain_j = 0;
    unsigned fused_tag = 0u;     // the newest k_lsmr_fused launch's tag: the one a reader that gave up leaves behind
    LsmrProf prof{{c->prof_ev[0].size(), c->prof_ev[1].size()}, {}};
    unsigned long long spins = 0;
    // cautious: the product workgroups wait for the decision before they stream
    auto launch_k1 = [&](bool cautious, bool commit) -> int {
        const int j = k1 + 1, in = (j - 1) & 1, out = j & 1;
        LsmrFused a;
        a.st_in = W.stb[in]; a.st_out = W.stb[out]; a.mail = c->d_mail;
        a.pu_in = W.fpu[in]; a.npu_in = W.fnpu + in; a.pu_out = W.fpu[out]; a.npu_out = W.fnpu + out;
        a.px_in = (W.damped && j > 1) ? W.pxb[in] : nullptr; a.npx_in = W.npxb[in];
        a.px_out = W.pxb[out]; a.npx_out = W.npxb[out];
        a.pv = W.pv; a.npv = W.npv;
        a.vt = W.vset; a.w = W.fw; a.P = s->d_P; a.dg = W.dgk;
        a.h_in = W.fh[in]; a.hbar_in = W.fhbar[in]; a.x_in = W.fx[in];
        a.h_out = W.fh[out]; a.hbar_out = W.fhbar[out]; a.x_out = W.fx[out];
        a.v = s->d_v; a.xout = W.d_x; a.ux = s->d_ux;
        a.uold = j == 1 ? W.d_y : s->d_u; a.unew = s->d_u;
        a.n = n; a.ub = ub;
        a.cautious = cautious ? 1 : 0;
        a.test_no_record = test_no_record;                      // (test hook: the in-launch hand-off fails)
        a.ho = W.fho;
        a.tag_prev = j > 1 ? fused_tag : 0u;
        if (++s->f3_tag == 0u) s->f3_tag = 1u;                  // a counter per solver (= per record buffer): every older record
        a.tag = s->f3_tag;                                      // carries another value; 0 is the zeroed buffer
        if (commit) {
            LSQ_LAUNCH(k_lsmr_commit_step<0>, dim3(lsq_div_up(n, LSQ_BIG_NT)), dim3(LSQ_BIG_NT), 0, c->stream, a, *tail->step);
            LSQ_HIP(hipGetLastError());
            return LSQ_OK;
        }
        fused_tag = a.tag;
        if (c->prof_kernels & 1) lsq_prof_mark(c, 0, 0);
        hipEvent_t e0, e1;
        if (lsq_prof_take(c, &e0, &e1)) {
            LSQ_LAUNCH_TIMED(k_lsmr_fused<0>, dim3(pb + ub), dim3(LSQ_BIG_NT), lds, c->stream, e0, e1, 0, sell_dev(S), S.wrows, m, nxpad, a);
            prof.iter[0].push_back(j);
        } else {
            LSQ_LAUNCH(k_lsmr_fused<0>, dim3(pb + ub), dim3(LSQ_BIG_NT), lds, c->stream, sell_dev(S), S.wrows, m, nxpad, a);
        }
        if (c->prof_kernels & 1) lsq_prof_mark(c, 0, 1);
        LSQ_HIP(hipGetLastError());
        ++k1;
        return LSQ_OK;
    };
    auto launch_k2 = [&]() -> int {      // K2 of iteration enq + 1 (its K1' is launch k1 == enq + 1)
        const int j = enq + 1, cur = j & 1;
        LsmrState *st = W.stb[cur];
        EpiV e2{&st->done, 0, st, W.fpu[cur], W.fnpu + cur, W.damped ? W.pxb[cur] : nullptr, W.npxb[cur], s->d_P, W.dgk,
                W.damped ? s->d_ux : nullptr, s->d_v, W.pv, W.npv, nullptr, 0.0, 0.0, 0, 0};
        e2.vout = W.vset; e2.cs = J->d_colscale; e2.wout = W.fw;
        if (c->prof_kernels & 2) lsq_prof_mark(c, 1, 0);
        const size_t before = c->prof_ev[1].size();
        LSQ_TRY(launch_sell_cols<false>(J, s->d_u, &st->done));
        if (c->prof_ev[1].size() > before) prof.iter[1].push_back(j);
        if (c->prof_kernels & 2) lsq_prof_mark(c, 1, 1);
        const int nb = lsq_div_up(n, LSQ_CMB_COLS);
        LSQ_LAUNCH((k_combine<EpiV>), dim3(std::min(nb, 2048)), dim3(LSQ_NT), 0, c->stream, J->scols.d_part, n, J->scols.ngw, e2, nb,
                   J->d_colscale);
        LSQ_HIP(hipGetLastError());
        ++enq;
        return LSQ_OK;
    };
    while (!r.finished) {
        const unsigned long long w = lsmr_progress_word(c);
        const LsmrProgress p(w, W.epoch);
        if (r.see(p)) break;
        if (wait_at > 0 && p.ours && r.it >= wait_at) {           // the cautious / commit launch found the solve unfinished
            if (wait_is_guess) {
                c->tail_spec[0]++;
                c->tail_spec[1]++;
                planned = 0;
            }
            if (commit_pending) {
                c->commit_step[1]++;
                commit_pending = false;
                plain_j = k1 + 1;
            }
            wait_at = 0;
        }
        if (W.dynamic && p.ours) {
            const int stop = pred.update(c->h_mail, w, r.it, W.atol, W.btol);
            if (stop > 0) planned = stop;
        }
        if (!(wait_at > 0 && r.it < wait_at)) {               // (else: a cautious launch is deciding iteration wait_at)
            if (k1 == enq + 1) {                                 // the rest of iteration enq + 1
                LSQ_TRY(launch_k2());
                spins = 0;
                continue;
            }
            // K1' number enq + 1 commits iteration enq: it does not count against the look-ahead (nothing is decided without it)
            if (enq - r.it < W.lookahead + 1 && enq < W.maxiter + 1) {
                // cautious: the launch that commits the planned last iteration (or the newest one, if the prediction names an
                // iteration whose commit is already in the queue) ...
                const bool guess = W.spec && planned > 0 && enq >= planned && enq >= 1;
                // ... and also where nothing is known yet: the launch that decides iteration 1, unless the previous solve was a
                // long one
                const bool unknown = W.spec && enq == 1 && pred.hint_it == 0 && tail->predict <= 3;
                if (k1 + 1 == plain_j) {                         // (a commit launch has just reported this iteration unfinished)
                    LSQ_TRY(launch_k1(false, false));
                } else {
                    const bool commit = commit_ok && (guess || unknown);
                    LSQ_TRY(launch_k1(guess || unknown, commit));
                    if (guess || unknown) {                      // nothing behind it until it has decided
                        wait_at = enq;
                        wait_is_guess = guess;
                        commit_pending = commit;
                    }
                }
                spins = 0;
                continue;
            }
        }
        if (c->idle_hook) lsq_run_idle_hook(c);
        if ((++spins & 0x3ffu) != 0) continue;
        // (a pending commit launch decides iteration k1 and, only if that ends the solve, leaves its state in set (k1 + 1) & 1)
        const int newest = commit_pending ? k1 + 1 : k1;
        LSQ_TRY(lsmr_stream_drained(c, W.epoch, newest - 1, W.stb[newest & 1], enq >= W.maxiter + 1, r));
        if (commit_pending && !r.finished && r.it < wait_at && hipStreamQuery(c->stream) == hipSuccess) {
            // (mailbox not visible, stream drained, no stop in that set: the commit launch found the solve unfinished)
            const LsmrProgress q(lsmr_progress_word(c), W.epoch);
            if (!(q.ours && (q.done || q.iter >= wait_at))) {
                LsmrState hs;
                LSQ_HIP(hipMemcpy(&hs, W.stb[k1 & 1], sizeof(hs), hipMemcpyDeviceToHost));
                if (hs.done) { r.it = hs.iter; r.istop = hs.istop; r.finished = true; }
                else {
                    if (wait_is_guess) { c->tail_spec[0]++; c->tail_spec[1]++; planned = 0; }
                    c->commit_step[1]++;
                    commit_pending = false;
                    plain_j = k1 + 1;
                    wait_at = 0;
                }
            }
        }
    }
    lsmr_drop_idle_samples(c, prof, r.it);
    if (r.istop == 99) {     // (a product workgroup gave up waiting for workgroup 0's record: lsq_lsmr3.h)
        lsq_set_error("lsmr: the in-launch hand-off of k_lsmr_fused timed out");
        return LSQ_EHIP;
    }
    // the launch that was to decide iteration wait_at is still the newest one: the stop is either that iteration's (a right guess)
    // or an EARLIER one's, committed by an older launch while this one was in the queue (a wrong guess: it then found a finished
    // solve, handed the state on and -- a commit launch -- took no step)
    if (wait_at > 0 && wait_is_guess) {
        c->tail_spec[0]++;
        if (r.it < wait_at) c->tail_spec[1]++;
    }
    if (commit_pending && r.it >= wait_at) {
        c->commit_step[0]++;
        *tail->step_taken = true;
    }
    return LSQ_OK;
}

// ---- four launches per inner iteration: K1 (J*v, EpiU) | K2 (J'u: k_sell_cols + k_combine<EpiV>, or the row-sharded form with
// the ranks' sum in the middle) | K3 (k_lsmr_update).  Row-sharded solves, wide n, unsliced layouts, LSQ_LSMR_FOUR_LAUNCHES=1.
// The caller's tail is PRE-PLACED (LsmrTail, lsq_solver.h): queued, guarded by the state's `notdone`, right behind the iteration
// that is planned to be the last -- first the caller's guess (the previous solve's count), from iteration 1 on the solve's own
// prediction (StopPredictor).
static int lsmr_run_four(const LsmrWork &W, StopPredictor &pred, LsmrRun &r) {
    lsq_solver *s = W.s; lsq_ctx *c = W.c; lsq_mat *J = W.J;
    const LsmrTail *tail = W.tail;
    const bool sharded = W.sharded;
    const int maxiter = W.maxiter;
    LsmrState *st = W.stb[0];
    EpiU eu{&st->done, 0, st, W.d_y, s->d_u, W.n, s->d_dg, s->d_t, s->d_ux, W.pu, W.npu, nullptr, 0.0};
    EpiV ev = lsmr_epi_v(W);
    ev.ux = W.damped ? s->d_ux : nullptr;
    int planned = W.spec ? tail->predict : 0;
    int tail_at = 0;             // iteration behind which the latest guarded tail was enqueued (0: none that is still undecided)
    int enq = 0;                 // whole iterations enqueued
    LsmrProf prof{{c->prof_ev[0].size(), c->prof_ev[1].size()}, {}};
    unsigned long long spins = 0;
    while (!r.finished) {
        const unsigned long long w = lsmr_progress_word(c);
        const LsmrProgress p(w, W.epoch);
        if (r.see(p)) break;
        if (W.spec && p.ours && tail_at > 0 && r.it >= tail_at) {   // (not done: `finished` left the loop above)
            // the tail behind iteration tail_at found the solve unfinished and skipped itself: a wrong guess
            c->tail_spec[0]++;
            c->tail_spec[1]++;
            tail_at = 0;
            planned = 0;
        }
        if (W.dynamic && p.ours) {
            const int stop = pred.update(c->h_mail, w, r.it, W.atol, W.btol);
            if (stop > 0 && tail_at == 0) planned = stop;
        }
        // the guarded tail: right behind the planned last iteration, as soon as that one is enqueued (or behind the newest
        // enqueued, still unreported one if the prediction names an iteration that is already in the queue)
        if (W.spec && tail_at == 0 && planned > 0 && enq >= planned && enq > r.it) {
            LSQ_TRY(tail->fn(&st->notdone, tail->user));
            tail_at = enq;
        }
        // Row-sharded: every rank must enqueue the SAME number of inner iterations (each carries a collective), so the count
        // cannot depend on when this host happens to see the mailbox: iterations go out in chunks of `lookahead`, and the
        // next chunk only once the last one has reported "not done" -- ceil(stop / lookahead) * lookahead on every rank.
        // (and the first chunk only once the SETUP has reported: a solve that is over before it starts -- A'b = 0 -- must not
        //  get a chunk on the ranks whose host looked too early)
        // (a speculative tail sits behind iteration tail_at: nothing more is queued until that iteration has reported)
        const bool hold = tail_at > 0 && enq == tail_at && r.it < tail_at;
        const bool want = sharded ? (p.ours && enq == r.it && enq < maxiter) : (!hold && enq - r.it < W.lookahead && enq < maxiter);
        if (want) {
            const int chunk = sharded ? (int)std::min<long long>(W.lookahead, (long long)maxiter - enq) : 1;
            for (int q = 0; q < chunk; ++q) {
                if (c->prof_kernels & 1) lsq_prof_mark(c, 0, 0);
                {
                    const size_t before = c->prof_ev[0].size();
                    LSQ_TRY(launch_product(J, 0, s->d_t, eu));   // K1
                    if (c->prof_ev[0].size() > before) prof.iter[0].push_back(enq + 1);
                }
                if (c->prof_kernels & 1) lsq_prof_mark(c, 0, 1);
                eu.uold = s->d_u;                            // after the first iteration u~ lives in d_u
                const int cur = enq & 1;                     // px buffer holding this iteration's sum(u~x^2)
                ev.px = W.damped ? W.pxb[cur] : nullptr;
                ev.npx = W.npxb[cur];
                if (c->prof_kernels & 2) lsq_prof_mark(c, 1, 0);
                {
                    const size_t before = c->prof_ev[1].size();
                    if (sharded) LSQ_TRY(rowshard_adjoint(s, J, s->d_u, ev, W.pu, W.npu));   // K2 with the ranks' sum in the middle
                    else LSQ_TRY(launch_product(J, 1, s->d_u, ev));   // K2
                    if (c->prof_ev[1].size() > before) prof.iter[1].push_back(enq + 1);
                }
                if (c->prof_kernels & 2) lsq_prof_mark(c, 1, 1);
                lsmr_launch_update(W, sharded, ev.px, ev.npx, cur ^ 1);   // K3
                LSQ_HIP(hipGetLastError());
                ++enq;
            }
            spins = 0;
            continue;
        }
        if (c->idle_hook) lsq_run_idle_hook(c);   // look-ahead window full: the device has work for a while
        if ((++spins & 0x3ffu) != 0) continue;
        LSQ_TRY(lsmr_stream_drained(c, W.epoch, enq, st, enq >= maxiter, r));
    }
    lsmr_drop_idle_samples(c, prof, r.it);
    // the latest guarded tail ran iff the solve was over when its kernels reached the device: stop iteration <= tail_at
    // (tails that skipped themselves were counted, as wrong guesses, when their iteration reported)
    if (tail_at > 0) {
        c->tail_spec[0]++;
        if (r.it > tail_at) c->tail_spec[1]++;
        else r.tail_ran = true;
    }
    return LSQ_OK;
}

int lsq_lsmr_solve(lsq_solver *s, lsq_mat *J, const double *d_y, double *d_damp, double *d_x, int *nmul,
                   const double *d_Jty, double y_sumsq, const LsmrLmPrep *lm, const LsmrTail *tail) {
    lsq_ctx *c = s->ctx;
    const int m = J->m, n = J->n;
    if (tail && tail->step_taken) *tail->step_taken = false;      // (only lsmr_run_fused ever sets it)
    if (m != s->m || n != s->n) {
        lsq_set_error("lsmr: solver allocated for %dx%d, Jacobian is %dx%d", s->m, s->n, m, n);
        return LSQ_EDIM;
    }
    if (s->gen_ldiv) {     // LSMR(preconditioner!, P) with a general P: the operator-level recurrence (lsq_lsmr_general.hip)
        if (s->row_cb) {
            lsq_set_error("row-sharded solves take diagonal preconditioners only");
            return LSQ_EARG;
        }
        LSQ_TRY(lsq_lsmr_general_solve(s, J, d_y, d_damp, d_x, nmul));
        s->last_lsmr_path = 4;
        return tail && tail->fn ? tail->fn(nullptr, tail->user) : LSQ_OK;
    }
    const bool sharded = s->row_cb != nullptr;     // J is a row block: the adjoint product is summed over the ranks
    if (lsq_small_mat(J) && !s->precond_cb && !sharded) {   // reference-order kernel
        LSQ_TRY(lsq_lsmr_exact_solve(s, J, d_y, d_damp, d_x, nmul));
        s->last_lsmr_path = 1;
        return tail && tail->fn ? tail->fn(nullptr, tail->user) : LSQ_OK;
    }
    LsmrWork W;
    W.s = s; W.c = c; W.J = J; W.d_y = d_y; W.d_x = d_x; W.m = m; W.n = n;
    W.damped = d_damp != nullptr; W.sharded = sharded;
    W.atol = 1e-6; W.btol = W.damped ? 0.5 : 1e-6; W.conlim = 1e8;      // lsmr.jl:54, il:255
    const long long rows = (sharded ? s->global_rows : (long long)m) + (W.damped ? n : 0);
    W.maxiter = (int)std::max<long long>(rows, n);                       // lsmr.jl:55
    W.lookahead = lsq_dbg_serial ? 1 : LSQ_LOOKAHEAD_DEFAULT;   // (serial debug mode: nothing queued behind an undecided iteration)
    W.epoch = (++c->mail_epoch) & 0x7fffffu;
    if (J->kind == LSQ_MAT_CSC) LSQ_TRY(lsq_ensure_csr(J));
    // The three-launch iteration (lsq_lsmr3.h): both sliced layouts, x resident in LDS, one rank.  Otherwise K1 | K2 | K3.
    const bool four_env = getenv("LSQ_LSMR_FOUR_LAUNCHES") != nullptr;      // (read per solve: the tests flip it)
    W.fused = !four_env && !sharded && J->kind == LSQ_MAT_CSC && J->srows.active && J->srows.ncw == 1 && J->scols.active &&
              n >= 1 && m >= 1 && c->num_cus >= 8;
    W.gn = nvec_grid(c, n); W.dgk = W.damped ? s->d_dg : nullptr;
    W.tail = tail;
    W.dynamic = tail && tail->fn && tail->dynamic && !sharded;
    W.spec = tail && tail->fn && !sharded && (tail->predict > 0 || W.dynamic);
    W.stb[0] = s->d_state; W.stb[1] = s->d_state + 1;
    W.pv = s->d_red + 4096;
    W.pxb[0] = s->d_red + 2 * 4096; W.pxb[1] = s->d_red + 3 * 4096;
    int *const counts = (int *)(s->d_red + 4 * 4096);               // npu, npv, npx[2]
    W.npv = counts + 1; W.npxb[0] = counts + 2; W.npxb[1] = counts + 3;
    double *const f3 = s->d_f3;
    W.fx[0] = s->d_rhs; W.fx[1] = f3; W.fhbar[0] = s->d_hbar; W.fhbar[1] = f3 + n; W.fh[0] = s->d_h; W.fh[1] = f3 + 2 * (size_t)n;
    W.fw = f3 + 3 * (size_t)n;
    W.fpu[0] = f3 + 4 * (size_t)n; W.fpu[1] = W.fpu[0] + 4096;
    W.fnpu = (int *)(W.fpu[1] + 4096); W.fho = (LsmrHandoff *)(W.fpu[1] + 4096 + 8);
    W.vset = W.fused ? s->d_t : s->d_v;
    W.pu = W.fused ? W.fpu[0] : s->d_red;
    W.npu = W.fused ? W.fnpu : counts;
    // computed once per Jacobian (reference: twice); row-sharded: the sum over the ranks' blocks -- the preconditioner is a
    // replicated n-vector and has to be the same on every rank
    const double *colsum = nullptr;
    LSQ_TRY(lsq_rowshard_colsum(s, J, &colsum));
    const int custom_p = s->precond_cb ? 1 : 0;
    if (custom_p) {   // preconditioner!(P, x, J, damp) on the host, damp still un-rooted (iterative_lsmr.jl:251-252)
        LSQ_HIP(hipStreamSynchronize(c->stream));
        if (s->precond_cb(s->d_P, J, d_damp, s->precond_user) != 0) {
            lsq_set_error("preconditioner callback reported failure");
            return LSQ_ECALLBACK;
        }
    }
    *(volatile unsigned long long *)c->h_mail = 0ull;
    LSQ_TRY(lsmr_enqueue_setup(W, d_damp, d_Jty, y_sumsq, lm, colsum, custom_p));

    StopPredictor pred{-1.0, -1.0, s->lsmr_ratio2, 0};
    LsmrRun r;
    LSQ_TRY(W.fused ? lsmr_run_fused(W, pred, r) : lsmr_run_four(W, pred, r));
    s->last_iter = r.it;
    s->last_istop = r.istop;
    s->last_lsmr_path = W.fused ? 3 : 2;
    if (nmul) *nmul = 2 * r.it;  // lsmr.jl:236 ch.mvps
    if (W.dynamic && pred.t2_prev > 0.0) s->lsmr_ratio2 = pred.ratio2;
    if (tail && tail->fn && !r.tail_ran) LSQ_TRY(tail->fn(nullptr, tail->user));
    return LSQ_OK;
}
