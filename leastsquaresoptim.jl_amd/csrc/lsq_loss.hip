// Robust losses and observation weights as a wrapper around the problem (include/lsqhip.h: lsq_loss_create).
// With z = f / sigma, a = |z| / c and the loss rho(a^2), the wrapped problem has the residual r~ = sign(z) c sqrt(rho) and the
// Jacobian diag(w / sigma) J, w = d r~ / d z: an exact least-squares problem (sum(abs2, r~) = c^2 sum(rho), J~'r~ = the gradient
// of that cost), so the loops, the solvers, central differences and the covariance entries take it unchanged.
// One elementwise kernel (k_loss_eval) and two callbacks that put it around the caller's own f! and g!.
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "lsq_common.h"

struct LsqLoss {
    lsq_ctx *ctx = nullptr;
    int kind = LSQ_LOSS_LINEAR;
    double scale = 1.0;
    int m = 0;
    double *d_sigma = nullptr;     // copy of the caller's sigmas (nullptr: none)
    double *d_raw = nullptr;       // the raw residual lsq_loss_g evaluates (m)
    double *d_rowf = nullptr;      // row factors w / sigma (m)
    unsigned *d_count = nullptr;   // rows with a > 1 of the last evaluation that asked for statistics
    lsq_f_callback f = nullptr;    // the inner problem (lsq_loss_set_problem)
    lsq_g_callback g = nullptr;
    void *user = nullptr;
};

// r~ and w of one row; the order of the operations is the specification (include/lsqhip.h) and the numpy twin's
// (api.py: loss_transform).  Every operation is one IEEE operation: the build has -ffp-contract=off.
template <int KIND>
__device__ __forceinline__ void loss_row(double z, double a, double c, double &rt, double &w) {
    rt = z;
    w = 1.0;
    if (KIND == LSQ_LOSS_LINEAR) return;
    if (!(a <= DBL_MAX)) {          // NaN and +-Inf pass through as they are: check_isfinite finds them where it would without a loss
        w = a != a ? 1.0 : 0.0;
        return;
    }
    if (KIND == LSQ_LOSS_HUBER) {
        if (a > 1.0) {
            const double q = a > 0x1p1022 ? 2.0 * sqrt(0.5 * a) : sqrt(2.0 * a - 1.0);   // (2a itself would overflow; the -1 is far below rounding there)
            rt = copysign(c * q, z);
            w = 1.0 / q;
        }
    } else if (KIND == LSQ_LOSS_SOFT_L1) {
        const double t = a > 0x1p500 ? a : sqrt(1.0 + a * a);
        const double q = sqrt(2.0 / (t + 1.0));
        rt = z * q;
        w = 1.0 / (t * q);
    } else {                        // LSQ_LOSS_CAUCHY
        if (a >= 0x1p-27) {
            const bool big = a > 0x1p500;
            const double L = big ? 2.0 * log(a) : log1p(a * a);
            const double q = sqrt(L) / a;
            rt = z * q;
            w = big ? (1.0 / (a * q)) / a : 1.0 / ((1.0 + a * a) * q);    // (1 / a^2 itself would underflow from a = 1e154 on)
        }
    }
}

// rt and f may be the same buffer (in place), so neither is __restrict__; any of rt / rowf / count may be null
template <int KIND>
__global__ void __launch_bounds__(LSQ_NT)
k_loss_eval(int m, const double *f, const double *__restrict__ sigma, double c, double *rt, double *__restrict__ rowf,
            unsigned *__restrict__ count) {
    __shared__ unsigned sh_count;
    if (threadIdx.x == 0) sh_count = 0;
    __syncthreads();
    unsigned outliers = 0;
    for (long long i = blockIdx.x * (long long)LSQ_NT + threadIdx.x; i < m; i += (long long)gridDim.x * LSQ_NT) {
        const double z = sigma ? f[i] / sigma[i] : f[i];
        const double a = fabs(z) / c;
        double r, w;
        loss_row<KIND>(z, a, c, r, w);
        outliers += a > 1.0;
        if (rt) rt[i] = r;
        if (rowf) rowf[i] = sigma ? w / sigma[i] : w;
    }
    if (count) {    // (integer counts: the order of the additions does not matter)
        if (outliers) atomicAdd(&sh_count, outliers);
        __syncthreads();
        if (threadIdx.x == 0 && sh_count) atomicAdd(count, sh_count);
    }
}

static int loss_eval_launch(LsqLoss *L, const double *d_f, double *d_rt, double *d_rowf, unsigned *d_count) {
    lsq_ctx *c = L->ctx;
    const int grid = std::min(lsq_div_up(L->m, LSQ_NT), c->num_cus * 16);
    switch (L->kind) {
    case LSQ_LOSS_LINEAR:
        LSQ_LAUNCH(k_loss_eval<LSQ_LOSS_LINEAR>, dim3(grid), dim3(LSQ_NT), 0, c->stream, L->m, d_f, (const double *)L->d_sigma,
                   L->scale, d_rt, d_rowf, d_count);
        break;
    case LSQ_LOSS_HUBER:
        LSQ_LAUNCH(k_loss_eval<LSQ_LOSS_HUBER>, dim3(grid), dim3(LSQ_NT), 0, c->stream, L->m, d_f, (const double *)L->d_sigma,
                   L->scale, d_rt, d_rowf, d_count);
        break;
    case LSQ_LOSS_SOFT_L1:
        LSQ_LAUNCH(k_loss_eval<LSQ_LOSS_SOFT_L1>, dim3(grid), dim3(LSQ_NT), 0, c->stream, L->m, d_f, (const double *)L->d_sigma,
                   L->scale, d_rt, d_rowf, d_count);
        break;
    default:
        LSQ_LAUNCH(k_loss_eval<LSQ_LOSS_CAUCHY>, dim3(grid), dim3(LSQ_NT), 0, c->stream, L->m, d_f, (const double *)L->d_sigma,
                   L->scale, d_rt, d_rowf, d_count);
        break;
    }
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

static void loss_free(LsqLoss *L) {
    hipFree(L->d_sigma);
    hipFree(L->d_raw);
    hipFree(L->d_rowf);
    hipFree(L->d_count);
    delete L;
}

extern "C" int lsq_loss_create(lsq_ctx *c, int kind, double scale, int m, const double *d_sigma_or_null, void **out) {
    if (!c || !out) {
        lsq_set_error("lsq_loss_create: null argument");
        return LSQ_EARG;
    }
    if (kind < LSQ_LOSS_LINEAR || kind > LSQ_LOSS_CAUCHY) {
        lsq_set_error("lsq_loss_create: unknown loss kind %d (0 linear, 1 huber, 2 soft_l1, 3 cauchy)", kind);
        return LSQ_EARG;
    }
    if (!(scale > 0.0 && scale <= DBL_MAX)) {
        lsq_set_error("lsq_loss_create: the loss scale must be finite and positive (got %g)", scale);
        return LSQ_EARG;
    }
    if (m < 1) {
        lsq_set_error("lsq_loss_create: needs m >= 1 residual rows (got %d)", m);
        return LSQ_EDIM;
    }
    LSQ_HIP(hipSetDevice(c->device));
    if (d_sigma_or_null) {      // one readback, here and never again
        std::vector<double> h(m);
        LSQ_TRY(lsq_d2h(c, h.data(), d_sigma_or_null, (size_t)m * sizeof(double)));
        for (int i = 0; i < m; ++i)
            if (!(h[i] > 0.0 && h[i] <= DBL_MAX)) {
                lsq_set_error("lsq_loss_create: sigma must be finite and positive, entry %d is %g", i, h[i]);
                return LSQ_EARG;
            }
    }
    LsqLoss *L = new LsqLoss();
    L->ctx = c;
    L->kind = kind;
    L->scale = scale;
    L->m = m;
    const size_t bytes = (size_t)m * sizeof(double);
    int st = LSQ_OK;
    if (hipMalloc(&L->d_raw, bytes) != hipSuccess || hipMalloc(&L->d_rowf, bytes) != hipSuccess ||
        hipMalloc(&L->d_count, sizeof(unsigned)) != hipSuccess ||
        (d_sigma_or_null && hipMalloc(&L->d_sigma, bytes) != hipSuccess)) {
        lsq_set_error("lsq_loss_create: out of device memory for %d rows", m);
        st = LSQ_EHIP;
    }
    if (st == LSQ_OK && d_sigma_or_null) st = lsq_d2d(c, L->d_sigma, d_sigma_or_null, bytes);
    if (st == LSQ_OK && hipStreamSynchronize(c->stream) != hipSuccess) st = LSQ_EHIP;   // the caller may free its sigmas now
    if (st != LSQ_OK) {
        (void)hipGetLastError();
        loss_free(L);
        return st;
    }
    *out = L;
    return LSQ_OK;
}

extern "C" int lsq_loss_destroy(void *loss) {
    if (!loss) return LSQ_OK;
    LsqLoss *L = (LsqLoss *)loss;
    hipStreamSynchronize(L->ctx->stream);
    loss_free(L);
    return LSQ_OK;
}

extern "C" int lsq_loss_set_problem(void *loss, lsq_f_callback f, lsq_g_callback g_or_null, void *user) {
    if (!loss || !f) {
        lsq_set_error("lsq_loss_set_problem: null argument");
        return LSQ_EARG;
    }
    LsqLoss *L = (LsqLoss *)loss;
    L->f = f;
    L->g = g_or_null;
    L->user = user;
    return LSQ_OK;
}

extern "C" int lsq_loss_eval(void *loss, const double *d_f, double *d_rt_or_null, double *d_rowfactor_or_null,
                             double *h_stats_or_null) {
    LSQ_RANGE("lsq_loss_eval");
    if (!loss || !d_f) {
        lsq_set_error("lsq_loss_eval: null argument");
        return LSQ_EARG;
    }
    LsqLoss *L = (LsqLoss *)loss;
    lsq_ctx *c = L->ctx;
    if (!h_stats_or_null) return loss_eval_launch(L, d_f, d_rt_or_null, d_rowfactor_or_null, nullptr);
    // the statistics need r~ somewhere: the object's own scratch when the caller wants no copy
    double *rt = d_rt_or_null ? d_rt_or_null : L->d_raw;
    LSQ_HIP(hipMemsetAsync(L->d_count, 0, sizeof(unsigned), c->stream));
    LSQ_TRY(loss_eval_launch(L, d_f, rt, d_rowfactor_or_null, L->d_count));
    LSQ_TRY(lsq_sumsq(c, L->m, rt, &h_stats_or_null[0]));       // (the reduction of the loops: their bits)
    unsigned count = 0;
    LSQ_TRY(lsq_d2h(c, &count, L->d_count, sizeof(unsigned)));
    h_stats_or_null[1] = (double)count;
    return LSQ_OK;
}

// The callbacks.  A failure leaves its reason in lsq_last_error and returns non-zero: the loop then reports LSQ_ECALLBACK.
static int loss_callback_failed() {
    lsq_keep_error_as_callback_reason();
    return 1;
}

static int loss_f(double *d_out, const double *d_x, void *user) {
    LsqLoss *L = (LsqLoss *)user;
    if (!L || !L->f) {
        lsq_set_error("lsq_loss_f: no problem behind the loss (pass the loss handle as user, after lsq_loss_set_problem)");
        return loss_callback_failed();
    }
    if (L->f(d_out, d_x, L->user) != 0) {
        lsq_set_error("lsq_loss_f: the inner f callback reported failure");
        return loss_callback_failed();
    }
    if (loss_eval_launch(L, d_out, d_out, nullptr, nullptr) != LSQ_OK) return loss_callback_failed();
    return 0;
}

static int loss_g(lsq_mat *J, const double *d_x, void *user) {
    LsqLoss *L = (LsqLoss *)user;
    if (!L || !L->f) {
        lsq_set_error("lsq_loss_g: no problem behind the loss (pass the loss handle as user, after lsq_loss_set_problem)");
        return loss_callback_failed();
    }
    if (!L->g) {
        lsq_set_error("lsq_loss_g: the problem has no g (hand the loop lsq_loss_f and a null g for central differences)");
        return loss_callback_failed();
    }
    if (!J || J->m != L->m) {
        lsq_set_error("lsq_loss_g: the Jacobian has %d rows, the loss was created for %d", J ? J->m : 0, L->m);
        return loss_callback_failed();
    }
    if (L->g(J, d_x, L->user) != 0) {
        lsq_set_error("lsq_loss_g: the inner g callback reported failure");
        return loss_callback_failed();
    }
    // the raw residual at THIS point (the batched loop hands g per-block points that no f call has seen): one evaluation
    // the loop does not count, like the closure of the reference's finite differences
    if (L->f(L->d_raw, d_x, L->user) != 0) {
        lsq_set_error("lsq_loss_g: the inner f callback reported failure");
        return loss_callback_failed();
    }
    if (loss_eval_launch(L, L->d_raw, nullptr, L->d_rowf, nullptr) != LSQ_OK) return loss_callback_failed();
    if (lsq_mat_scale_rows(J, L->d_rowf) != LSQ_OK) return loss_callback_failed();   // (its own reason stands)
    return 0;
}

extern "C" lsq_f_callback lsq_loss_f(void) { return loss_f; }
extern "C" lsq_g_callback lsq_loss_g(void) { return loss_g; }
