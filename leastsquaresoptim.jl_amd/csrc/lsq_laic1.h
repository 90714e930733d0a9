// dlaic1, the incremental condition estimation behind xGELSY's rank decision: shared by the dense QR kernels (lsq_qr.hip)
// and the per-block QR on block-diagonal Jacobians (lsq_blockqr.hip).
#pragma once
#include <cfloat>
#include <cmath>

#include <hip/hip_runtime.h>

// LAPACK dlaic1 (incremental condition estimation); alpha = x'w is supplied by the caller.
__device__ inline void laic1_dev(int job, double alpha, double sest, double gamma, double *sestpr, double *s,
                          double *c) {
    const double eps = DBL_EPSILON / 2;
    double absalp = fabs(alpha), absgam = fabs(gamma), absest = fabs(sest);
    double s1, s2, tmp, b, cc, t, zeta1, zeta2, sine, cosine;
    if (job == 1) {
        if (sest == 0.0) {
            s1 = fmax(absgam, absalp);
            if (s1 == 0.0) { *s = 0; *c = 1; *sestpr = 0; }
            else { *s = alpha / s1; *c = gamma / s1; tmp = sqrt(*s * *s + *c * *c); *s /= tmp; *c /= tmp; *sestpr = s1 * tmp; }
        } else if (absgam <= eps * absest) {
            *s = 1; *c = 0; tmp = fmax(absest, absalp); s1 = absest / tmp; s2 = absalp / tmp;
            *sestpr = tmp * sqrt(s1 * s1 + s2 * s2);
        } else if (absalp <= eps * absest) {
            s1 = absgam; s2 = absest;
            if (s1 <= s2) { *s = 1; *c = 0; *sestpr = s2; } else { *s = 0; *c = 1; *sestpr = s1; }
        } else if (absest <= eps * absalp || absest <= eps * absgam) {
            s1 = absgam; s2 = absalp;
            if (s1 <= s2) { tmp = s1 / s2; *s = sqrt(1 + tmp * tmp); *sestpr = s2 * *s; *c = (gamma / s2) / *s; *s = copysign(1.0, alpha) / *s; }
            else { tmp = s2 / s1; *c = sqrt(1 + tmp * tmp); *sestpr = s1 * *c; *s = (alpha / s1) / *c; *c = copysign(1.0, gamma) / *c; }
        } else {
            zeta1 = alpha / absest; zeta2 = gamma / absest;
            b = (1 - zeta1 * zeta1 - zeta2 * zeta2) * 0.5; cc = zeta1 * zeta1;
            t = b > 0 ? cc / (b + sqrt(b * b + cc)) : sqrt(b * b + cc) - b;
            sine = -zeta1 / t; cosine = -zeta2 / (1 + t);
            tmp = sqrt(sine * sine + cosine * cosine);
            *s = sine / tmp; *c = cosine / tmp; *sestpr = sqrt(t + 1) * absest;
        }
    } else {
        if (sest == 0.0) {
            *sestpr = 0;
            if (fmax(absgam, absalp) == 0.0) { sine = 1; cosine = 0; } else { sine = -gamma; cosine = alpha; }
            s1 = fmax(fabs(sine), fabs(cosine));
            *s = sine / s1; *c = cosine / s1; tmp = sqrt(*s * *s + *c * *c); *s /= tmp; *c /= tmp;
        } else if (absgam <= eps * absest) {
            *s = 0; *c = 1; *sestpr = absgam;
        } else if (absalp <= eps * absest) {
            s1 = absgam; s2 = absest;
            if (s1 <= s2) { *s = 0; *c = 1; *sestpr = s1; } else { *s = 1; *c = 0; *sestpr = s2; }
        } else if (absest <= eps * absalp || absest <= eps * absgam) {
            s1 = absgam; s2 = absalp;
            if (s1 <= s2) { tmp = s1 / s2; *c = sqrt(1 + tmp * tmp); *sestpr = absest * (tmp / *c); *s = -(gamma / s2) / *c; *c = copysign(1.0, alpha) / *c; }
            else { tmp = s2 / s1; *s = sqrt(1 + tmp * tmp); *sestpr = absest / *s; *c = (alpha / s1) / *s; *s = -copysign(1.0, gamma) / *s; }
        } else {
            zeta1 = alpha / absest; zeta2 = gamma / absest;
            double norma = fmax(1 + zeta1 * zeta1 + fabs(zeta1 * zeta2), fabs(zeta1 * zeta2) + zeta2 * zeta2);
            double test = 1 + 2 * (zeta1 - zeta2) * (zeta1 + zeta2);
            if (test >= 0) {
                b = (zeta1 * zeta1 + zeta2 * zeta2 + 1) * 0.5; cc = zeta2 * zeta2;
                t = cc / (b + sqrt(fabs(b * b - cc)));
                sine = zeta1 / (1 - t); cosine = -zeta2 / t;
                *sestpr = sqrt(t + 4 * eps * eps * norma) * absest;
            } else {
                b = (zeta2 * zeta2 + zeta1 * zeta1 - 1) * 0.5; cc = zeta1 * zeta1;
                t = b >= 0 ? -cc / (b + sqrt(b * b + cc)) : b - sqrt(b * b + cc);
                sine = -zeta1 / t; cosine = -zeta2 / (1 + t);
                *sestpr = sqrt(1 + t + 4 * eps * eps * norma) * absest;
            }
            tmp = sqrt(sine * sine + cosine * cosine);
            *s = sine / tmp; *c = cosine / tmp;
        }
    }
}
