// Output-side kernels of the warped GP (GPy/GPy/models/warped_gp.py:13-160, GPy/GPy/util/warping_functions.py:71-169): the warp
// of the targets with its log-Jacobian, the warp's LML gradient, the inverse, and the Gauss-Hermite moments of a prediction
// pushed back through the inverse.  Elementwise work over vectors that are resident already; the arithmetic is warp_math.h's.
// Every reduction has a fixed order and no floating-point atomics: the same input gives the same bits on every call.
#include "warp_math.h"
#include "../../include/gphip.h"

#define WARP_NT 1024   // threads of the one workgroup that warps the targets and sums log f' over them
#define WARP_GRAD_NT 256   // ... and of the one that takes the gradient sums: 25 running sums a thread, all in registers

__device__ __forceinline__ double wp_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}
// sum over the workgroup's NT threads, lane 0 of each wave in wave order; every thread gets it
template <int NT>
__device__ __forceinline__ double wp_block_sum(double v, double *sh) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    v = wp_wave_sum(v);
    if (lane == 0) sh[wv] = v;
    __syncthreads();
    double r = 0.0;
    for (int i = 0; i < NT / 64; ++i) r += sh[i];
    __syncthreads();
    return r;
}

// ---- Y <- f(Y_raw) and sum_n log f'(y_n)  (WarpedGP.transform_data / log_likelihood, warped_gp.py:47-57) ----------------------
// One workgroup: thread t takes observations t, t + WARP_NT, ... in order.
__device__ __forceinline__ void warp_y_body(const double *Yraw, long N, const WarpParams &w, double *Y, double *logjac) {
    __shared__ double sh[WARP_NT / 64];
    double s = 0.0;
    for (long i = threadIdx.x; i < N; i += WARP_NT) {
        double f, df;
        warp_f_df(w, Yraw[i], f, df);
        Y[i] = f;
        s += log(df);
    }
    s = wp_block_sum<WARP_NT>(s, sh);
    if (threadIdx.x == 0) logjac[0] = s;
}
__global__ __launch_bounds__(WARP_NT) void warp_y_kernel(const double *Yraw, long N, WarpParams w, double *Y, double *logjac) {
    warp_y_body(Yraw, N, w, Y, logjac);
}
// member z = blockIdx.x of gp_fit_grad_warp_batch, one workgroup each: the shared raw targets through the member's warp wt[z]
// (device table) into its target block Y + z sY, sum log f_z' into logjac[z so]
__global__ __launch_bounds__(WARP_NT) void warp_y_batch_kernel(const double *Yraw, long N, const WarpParams *__restrict__ wt, double *Y, long sY,
                                                               double *logjac, long so) {
    const long z = blockIdx.x;
    const WarpParams &w = wt[z];   // (read in place: a private copy is indexed by the term and would live in scratch)
    warp_y_body(Yraw, N, w, Y + z * sY, logjac + z * so);
}
void launch_warp_y(hipStream_t s, const double *Yraw, long N, const WarpParams &w, double *Y, double *logjac) {
    GP_LAUNCH(warp_y_kernel, dim3(1), dim3(WARP_NT), 0, s, Yraw, N, w, Y, logjac);
}
void launch_warp_y_members(hipStream_t s, const double *Yraw, long N, const WarpParams *wt, double *Y, long sY, double *logjac,
                           long so, int nb) {
    GP_LAUNCH(warp_y_batch_kernel, dim3((unsigned)nb), dim3(WARP_NT), 0, s, Yraw, N, wt, Y, sY, logjac, so);
}

// ---- the 3 T + 1 sums of TanhFunction.update_grads (warping_functions.py:159-169) ------------------------------------------------
// out[(a_0, b_0, c_0, a_1, ..., d)]; one workgroup, per-thread sums in observation order, then one workgroup sum per parameter.
__device__ __forceinline__ void warp_grad_body(const double *Yraw, const double *alpha, long N, const WarpParams &w, double *out) {
    __shared__ double sh[WARP_GRAD_NT / 64];
    double g[GP_WARP_NPSI];
#pragma unroll
    for (int q = 0; q < GP_WARP_NPSI; ++q) g[q] = 0.0;
    for (long i = threadIdx.x; i < N; i += WARP_GRAD_NT) warp_grad_terms(w, Yraw[i], alpha[i], g);
#pragma unroll
    for (int q = 0; q < GP_WARP_NPSI - 1; ++q) {
        if (q < 3 * w.n) {   // (uniform: every thread of the workgroup takes part in the sums it reaches)
            const double v = wp_block_sum<WARP_GRAD_NT>(g[q], sh);
            if (threadIdx.x == 0) out[q] = v;
        }
    }
    const double vd = wp_block_sum<WARP_GRAD_NT>(g[GP_WARP_NPSI - 1], sh);   // d: the last slot of the sums, behind the terms in out
    if (threadIdx.x == 0) out[3 * w.n] = vd;
}
__global__ __launch_bounds__(WARP_GRAD_NT) void warp_grad_kernel(const double *Yraw, const double *alpha, long N, WarpParams w,
                                                                 double *out) {
    warp_grad_body(Yraw, alpha, N, w, out);
}
// member z = blockIdx.x of gp_fit_grad_warp_batch, one workgroup each: its alpha + z sV and warp wt[z], sums at out + z so
__global__ __launch_bounds__(WARP_GRAD_NT) void warp_grad_batch_kernel(const double *Yraw, const double *alpha, long sV, long N,
                                                                       const WarpParams *__restrict__ wt, double *out, long so) {
    const long z = blockIdx.x;
    const WarpParams &w = wt[z];   // (read in place: a private copy is indexed by the term and would live in scratch)
    warp_grad_body(Yraw, alpha + z * sV, N, w, out + z * so);
}
void launch_warp_grad(hipStream_t s, const double *Yraw, const double *alpha, long N, const WarpParams &w, double *out) {
    GP_LAUNCH(warp_grad_kernel, dim3(1), dim3(WARP_GRAD_NT), 0, s, Yraw, alpha, N, w, out);
}
void launch_warp_grad_members(hipStream_t s, const double *Yraw, const double *alpha, long sV, long N, const WarpParams *wt,
                              double *out, long so, int nb) {
    GP_LAUNCH(warp_grad_batch_kernel, dim3((unsigned)nb), dim3(WARP_GRAD_NT), 0, s, Yraw, alpha, sV, N, wt, out, so);
}

// ---- y = f^-1(z), one element per lane (predict_quantiles, warped_gp.py:118-132) -------------------------------------------------
__global__ __launch_bounds__(256) void warp_inverse_kernel(const double *z, long n, WarpParams w, double *y) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    y[i] = warp_inv(w, warp_sum_a(w), z[i]);
}
void launch_warp_inverse(hipStream_t s, const double *z, long n, const WarpParams &w, double *y) {
    GP_LAUNCH(warp_inverse_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, z, n, w, y);
}

// ---- Gauss-Hermite moments of a prediction in the space of the observations (WarpedGP.predict, warped_gp.py:62-116) ------------
// One (candidate, node) pair per lane; a candidate's G nodes (G = deg rounded up to a power of two, at most 64) sit in
// adjacent lanes of one wave, G-aligned, and are summed by an exclusive-or butterfly over those lanes alone: a fixed tree whose
// shape depends on G only, so a candidate's result depends neither on M nor on its row.  Lanes beyond deg carry weight 0, lanes
// beyond the last candidate repeat it and store nothing (every lane of a wave reaches every shuffle).
//   m = mean y_std + y_mean, sigma = sqrt(max(var, 0)) y_std   (the affine un-normalisation first, warped_gp.py:101)
//   y_k = f^-1(m + sqrt2 sigma t_k);  wmean = sum w_k y_k / sqrt(pi);  wvar = sum w_k y_k^2 / sqrt(pi) - wmean^2
//   median = f^-1(m);  partials (d wmean / d m, d wmean / d sigma, d wvar / d m, d wvar / d sigma) from
//   d y_k / d m = 1 / f'(y_k), d y_k / d sigma = sqrt2 t_k / f'(y_k).
__global__ __launch_bounds__(256) void warp_moments_kernel(const double *mean, const double *var, long M, double y_mean,
                                                           double y_std, WarpParams w, WarpNodes gh, int G, double *wmean,
                                                           double *wvar, double *median, double *partials) {
    const int per_block = 256 / G;
    const int k = threadIdx.x & (G - 1);
    long c = (long)blockIdx.x * per_block + threadIdx.x / G;
    const bool live = c < M;
    c = live ? c : M - 1;
    const double sqrt2 = 1.41421356237309504880168872420970, inv_sqrt_pi = 0.56418958354775628694807945156077;
    const double m = mean[c] * y_std + y_mean;
    const double v = var[c];
    const double sigma = sqrt(v > 0.0 ? v : (v == v ? 0.0 : v)) * y_std;   // (a NaN variance stays NaN)
    const bool node = k < gh.deg;
    const double t = node ? gh.t[node ? k : 0] : 0.0, wt = node ? gh.w[node ? k : 0] : 0.0;
    const double sum_a = warp_sum_a(w);
    const double y = warp_inv(w, sum_a, m + sqrt2 * sigma * t);
    double s[6];
    s[0] = wt * y;
    s[1] = wt * y * y;
    if (partials) {
        double f, fp;
        warp_f_df(w, y, f, fp);
        const double dm = wt / fp, ds = dm * (sqrt2 * t);
        s[2] = dm;
        s[3] = ds;
        s[4] = 2.0 * y * dm;
        s[5] = 2.0 * y * ds;
    } else {
        s[2] = s[3] = s[4] = s[5] = 0.0;
    }
    const int nsum = partials ? 6 : 2;
    for (int o = G >> 1; o > 0; o >>= 1) {
#pragma unroll
        for (int q = 0; q < 6; ++q)
            if (q < nsum) s[q] += __shfl_xor(s[q], o);   // (uniform: partials is the launch's)
    }
    if (!live || k != 0) return;
    const double wm = s[0] * inv_sqrt_pi;
    wmean[c] = wm;
    wvar[c] = s[1] * inv_sqrt_pi - wm * wm;
    if (median) median[c] = warp_inv(w, sum_a, m);
    if (partials) {
        const double dm_dm = s[2] * inv_sqrt_pi, dm_ds = s[3] * inv_sqrt_pi;
        partials[4 * c + 0] = dm_dm;
        partials[4 * c + 1] = dm_ds;
        partials[4 * c + 2] = s[4] * inv_sqrt_pi - 2.0 * wm * dm_dm;
        partials[4 * c + 3] = s[5] * inv_sqrt_pi - 2.0 * wm * dm_ds;
    }
}
int warp_group_lanes(int deg) {
    int G = 1;
    while (G < deg) G <<= 1;
    return G;
}
void launch_warp_moments(hipStream_t s, const double *mean, const double *var, long M, double y_mean, double y_std,
                         const WarpParams &w, const WarpNodes &gh, double *wmean, double *wvar, double *median, double *partials) {
    const int G = warp_group_lanes(gh.deg);
    const long per_block = 256 / G;
    GP_LAUNCH(warp_moments_kernel, dim3((unsigned)((M + per_block - 1) / per_block)), dim3(256), 0, s, mean, var, M, y_mean, y_std,
              w, gh, G, wmean, wvar, median, partials);
}
