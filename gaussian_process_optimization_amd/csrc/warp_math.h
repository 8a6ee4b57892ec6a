// The output warp of the warped GP as host / device functions, shared by the kernels (warp.hip) and the entry points
// (api_warp.hip): f, f', the parameter partials and the inverse of
//   f(y) = d y + sum_i a_i tanh(b_i (y + c_i))      (Snelson et al.; TanhFunction, GPy/GPy/util/warping_functions.py:71-169).
// Valid parameters are finite with a_i >= 0, b_i >= 0 and d > 0: f' >= d > 0, so f is strictly increasing.
#pragma once
#include "gphip_internal.h"

#define GP_WARP_MAX_TERMS 8     // tanh terms of one warp
#define GP_WARP_MAX_DEG 64      // Gauss-Hermite nodes of one prediction: the nodes of a candidate share a wave
#define GP_WARP_NPSI (3 * GP_WARP_MAX_TERMS + 1)   // parameters of the largest warp: (a, b, c) per term, then d
#define GP_WARP_INV_ITERS 128   // cap of the inverse's iteration; bisection alone ends inside it (see warp_inv)

// The parameters, by value in every kernel's arguments.  n = 0 is the identity (the warp is off): d is then 1.
struct WarpParams {
    int n;
    double d;
    double a[GP_WARP_MAX_TERMS], b[GP_WARP_MAX_TERMS], c[GP_WARP_MAX_TERMS];
};

// Gauss-Hermite nodes and weights of a prediction (numpy.polynomial.hermite.hermgauss on the host), by value as well
struct WarpNodes {
    int deg;
    double t[GP_WARP_MAX_DEG], w[GP_WARP_MAX_DEG];
};

__host__ __device__ inline bool warp_params_valid(const WarpParams &w) {
    if (w.n < 0 || w.n > GP_WARP_MAX_TERMS) return false;
    if (!(w.d > 0.0) || !(w.d <= 1.7976931348623157e308)) return false;
    for (int i = 0; i < w.n; ++i) {
        if (!(w.a[i] >= 0.0) || !(w.a[i] <= 1.7976931348623157e308)) return false;
        if (!(w.b[i] >= 0.0) || !(w.b[i] <= 1.7976931348623157e308)) return false;
        if (!(fabs(w.c[i]) <= 1.7976931348623157e308)) return false;
    }
    return true;
}

__host__ __device__ inline double warp_sum_a(const WarpParams &w) {
    double s = 0.0;
    for (int i = 0; i < w.n; ++i) s += w.a[i];
    return s;
}

// f(y), in the reference's order of operations (warping_functions.py:93-106), and f'(y) = d + sum_i a_i b_i (1 - r_i^2),
// r_i = tanh(b_i (y + c_i))   (fgrad_y, :108-128)
__host__ __device__ inline void warp_f_df(const WarpParams &w, double y, double &f, double &df) {
    f = w.d * y;
    df = w.d;
    for (int i = 0; i < w.n; ++i) {
        const double r = tanh(w.b[i] * (y + w.c[i]));
        f += w.a[i] * r;
        df += w.a[i] * w.b[i] * (1.0 - r * r);
    }
}

// One observation's share of the warp's LML gradient (TanhFunction.update_grads, warping_functions.py:159-169):
//   g[psi] += -alpha df/dpsi(y) + (df'/dpsi)(y) / f'(y),   g[GP_WARP_NPSI] laid out (a_0, b_0, c_0, a_1, ...) with d LAST, at
//   g[GP_WARP_NPSI - 1] whatever the number of terms (fixed slots: the sums stay in registers)
// with s_i = b_i (y + c_i), r_i = tanh s_i, q_i = 1 - r_i^2:
//   a_i: df = r_i                 df' = b_i q_i
//   b_i: df = a_i (y + c_i) q_i   df' = a_i q_i (1 - 2 s_i r_i)
//   c_i: df = a_i b_i q_i         df' = -2 a_i b_i^2 r_i q_i
//   d  : df = y                   df' = 1
__host__ __device__ inline void warp_grad_terms(const WarpParams &w, double y, double alpha, double *g) {
    double f, fp;
    warp_f_df(w, y, f, fp);
    const double ifp = 1.0 / fp;
#pragma unroll
    for (int i = 0; i < GP_WARP_MAX_TERMS; ++i) {
        if (i < w.n) {
            const double a = w.a[i], b = w.b[i], yc = y + w.c[i];
            const double s = b * yc, r = tanh(s), q = 1.0 - r * r;
            g[3 * i + 0] += -alpha * r + (b * q) * ifp;
            g[3 * i + 1] += -alpha * (a * yc * q) + (a * q * (1.0 - 2.0 * s * r)) * ifp;
            g[3 * i + 2] += -alpha * (a * b * q) + (-2.0 * a * b * b * r * q) * ifp;
        }
    }
    g[GP_WARP_NPSI - 1] += -alpha * y + ifp;
}

// y = f^-1(z): Newton's iteration kept inside a bracket.  f - d y lies in [-sum a, sum a], so the root -- unique, f being
// strictly increasing -- lies in [(z - sum a) / d, (z + sum a) / d]; every iterate moves one end of the bracket to itself.  A
// Newton step that leaves the bracket, or that does not at least halve the previous step, is replaced by the bracket's
// midpoint, so the iteration ends for every valid parameter set however flat f is between its steps (the reference's damped
// iteration, warping_functions.py:34-57, does not: it is NOT reproduced, nor is its stopping rule over the whole array).  It
// stops when the step is below 2^-52 max(1, |y|), at f(y) == z, or at GP_WARP_INV_ITERS; the trip count depends on the lane's
// own z alone, so a lane's result does not depend on its company, and no lane can spin.  A non-finite z is returned as it is.
__host__ __device__ inline double warp_inv(const WarpParams &w, double sum_a, double z) {
    if (w.n == 0) return z / w.d;
    if (!(fabs(z) <= 1.7976931348623157e308)) return z;
    double lo = (z - sum_a) / w.d, hi = (z + sum_a) / w.d;
    double y = z / w.d, dxold = hi - lo;
    for (int it = 0; it < GP_WARP_INV_ITERS; ++it) {
        double f, df;
        warp_f_df(w, y, f, df);
        f -= z;
        if (f == 0.0) break;
        if (f > 0.0) hi = y; else lo = y;
        double dx = f / df, yn = y - dx;
        if (!(yn > lo && yn < hi) || fabs(2.0 * f) > fabs(dxold * df)) {
            yn = 0.5 * (lo + hi);
            dx = y - yn;
        }
        dxold = dx;
        y = yn;
        if (fabs(dx) <= 2.220446049250313e-16 * fmax(1.0, fabs(y))) break;
    }
    return y;
}

// ---- warp.hip ---------------------------------------------------------------------------------------------------------------
// Y[i] = f(Yraw[i]), i < N, and logjac[0] = sum_i log f'(Yraw[i])
void launch_warp_y(hipStream_t s, const double *Yraw, long N, const WarpParams &w, double *Y, double *logjac);
// out[3 n + 1] = sum_i of warp_grad_terms(Yraw[i], alpha[i])
void launch_warp_grad(hipStream_t s, const double *Yraw, const double *alpha, long N, const WarpParams &w, double *out);
// the two above for nb members, one workgroup each (gp_fit_grad_warp_batch): member z warps the SHARED raw targets with wt[z]
// (device table) into Y + z sY, log-Jacobian at logjac[z so]; its gradient sums from alpha + z sV go to out + z so
void launch_warp_y_members(hipStream_t s, const double *Yraw, long N, const WarpParams *wt, double *Y, long sY, double *logjac,
                           long so, int nb);
void launch_warp_grad_members(hipStream_t s, const double *Yraw, const double *alpha, long sV, long N, const WarpParams *wt,
                              double *out, long so, int nb);
void launch_warp_inverse(hipStream_t s, const double *z, long n, const WarpParams &w, double *y);
// warped mean / variance [M] of the Gaussians (mean, var) [M] (device pointers); median [M] and partials [M, 4] may be null
void launch_warp_moments(hipStream_t s, const double *mean, const double *var, long M, double y_mean, double y_std,
                         const WarpParams &w, const WarpNodes &gh, double *wmean, double *wvar, double *median, double *partials);
