// GP classification by Laplace's method with a probit link: the kernels of one Newton step and of the marginal's gradient
// (host side: api_laplace.hip).  Rasmussen & Williams, Gaussian Processes for Machine Learning, Algorithms 3.1 and 5.1.
//
// Labels y in {-1, +1}, z = y f, n(z) = phi(z) / Phi(z):
//   log p = log Phi(z),  g = y n,  W = n (n + z) floored at LAP_W_FLOOR,  t = y [n (z^2 - 1) + 3 z n^2 + 2 n^3]
// n is formed in log space as feas_terms (acq_math.h) forms it, so it stays finite (~ -z) where Phi underflows.
//
// Every vector kernel is fixed-order: a row's dot product is one wavefront's strided partial sums folded by __shfl_down, the
// scalar sums are one workgroup's.  No atomics anywhere: the same inputs give the same bits.
#include "gphip_internal.h"
#include "../../include/gphip.h"
#include "acq_math.h"

#define LAP_W_FLOOR 1e-20

__device__ __forceinline__ double lap_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}
// sum over a 1024-thread workgroup in a fixed order (sh: 16 doubles); every thread gets the result
__device__ __forceinline__ double lap_block_sum(double v, double *sh) {
    v = lap_wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0.0;
    for (int i = 0; i < 16; ++i) r += sh[i];
    __syncthreads();
    return r;
}
__device__ __forceinline__ double lap_block_max(double v, double *sh) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = sh[0];
    for (int i = 1; i < 16; ++i) r = fmax(r, sh[i]);
    __syncthreads();
    return r;
}

// the probit site at latent value f under label y
__device__ __forceinline__ void lap_site(double y, double f, double &logp, double &g, double &W, double &t) {
    const double z = y * f;
    logp = gp_log_ndtr(z);
    const double n = exp(-0.5 * z * z - 0.91893853320467274178032973640562 - logp);
    g = y * n;
    const double w = n * (n + z);
    W = (w < LAP_W_FLOOR) ? LAP_W_FLOOR : w;
    t = y * (n * (z * z - 1.0) + 3.0 * z * (n * n) + 2.0 * (n * n * n));
}

// W, sqrt W, b = W f + g and t at f, for the N rows (the padding up to Npad: W = sqrt W = 1, b = t = 0)
__global__ __launch_bounds__(256) void lap_site_kernel(const double *y, const double *f, long N, long Npad, double *W, double *sw,
                                                       double *b, double *t) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= Npad) return;
    if (i >= N) {
        W[i] = sw[i] = 1.0;
        b[i] = t[i] = 0.0;
        return;
    }
    double logp, g, w, tt;
    lap_site(y[i], f[i], logp, g, w, tt);
    W[i] = w;
    sw[i] = sqrt(w);
    b[i] = fma(w, f[i], g);
    t[i] = tt;
}
void launch_lap_site(hipStream_t s, const double *y, const double *f, long N, long Npad, double *W, double *sw, double *b, double *t) {
    GP_LAUNCH(lap_site_kernel, dim3((unsigned)((Npad + 255) / 256)), dim3(256), 0, s, y, f, N, Npad, W, sw, b, t);
}

// out_i = scale_i sum_{j < N} M[i, j] v_j for i < N (scale null: 1), or, with `from`, out_i = from_i - that sum.  One wavefront
// per row, four rows per workgroup
__global__ __launch_bounds__(256) void lap_matvec_kernel(const double *M, long ld, const double *v, long N, const double *scale,
                                                         const double *from, double *out) {
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    const int lane = threadIdx.x & 63;
    const double *row = M + i * ld;
    double s = 0.0;
    for (long j = lane; j < N; j += 64) s = fma(row[j], v[j], s);
    s = lap_wave_sum(s);
    if (lane == 0) {
        if (scale) s *= scale[i];
        out[i] = from ? from[i] - s : s;
    }
}
void launch_lap_matvec(hipStream_t s, const double *M, long ld, const double *v, long N, const double *scale, const double *from,
                       double *out) {
    GP_LAUNCH(lap_matvec_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, M, ld, v, N, scale, from, out);
}

// B = I + W^1/2 K W^1/2 into the lower tiles of A (whole 128 x 128 tiles, as the K-build writes them; identity in the padding)
// from the full K beside it.  Two columns a thread
__global__ __launch_bounds__(256) void lap_bbuild_kernel(double *A, long lda, const double *K, long ldk, const double *sw, long N,
                                                         long Npad) {
    const long j = ((long)blockIdx.x * 256 + threadIdx.x) * 2, i = blockIdx.y;
    if (j >= Npad || j / GP_TILE > i / GP_TILE) return;
    double2_t o;
    if (i < N) {
        const double2_t k = *(const double2_t *)(K + i * ldk + j);
        const double si = sw[i];
        o[0] = (j < N) ? (si * k[0]) * sw[j] : 0.0;
        o[1] = (j + 1 < N) ? (si * k[1]) * sw[j + 1] : 0.0;
        if (j == i) o[0] += 1.0;
        if (j + 1 == i) o[1] += 1.0;
    } else {
        o[0] = (j == i) ? 1.0 : 0.0;
        o[1] = (j + 1 == i) ? 1.0 : 0.0;
    }
    *(double2_t *)(A + i * lda + j) = o;
}
void launch_lap_bbuild(hipStream_t s, double *A, long lda, const double *K, long ldk, const double *sw, long N, long Npad) {
    GP_LAUNCH(lap_bbuild_kernel, dim3((unsigned)((Npad / 2 + 255) / 256), (unsigned)Npad), dim3(256), 0, s, A, lda, K, ldk, sw, N,
              Npad);
}

// da = (b - sqrt W . w) - a: the Newton direction in a (zeros in the padding)
__global__ __launch_bounds__(256) void lap_dir_kernel(const double *b, const double *sw, const double *w, const double *a, long N,
                                                      long Npad, double *da) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= Npad) return;
    da[i] = (i < N) ? (b[i] - sw[i] * w[i]) - a[i] : 0.0;
}
void launch_lap_dir(hipStream_t s, const double *b, const double *sw, const double *w, const double *a, long N, long Npad, double *da) {
    GP_LAUNCH(lap_dir_kernel, dim3((unsigned)((Npad + 255) / 256)), dim3(256), 0, s, b, sw, w, a, N, Npad, da);
}

// The objective along the step, one workgroup: with a' = a + step da and f' = f + step df,
//   res[0] = psi = -1/2 a' . f' + sum log Phi(y f'),  res[1] = -1/2 a' . f',  res[2] = sum log Phi(y f'),
//   res[3] = max |da|,  res[4] = max |a'|
__global__ __launch_bounds__(1024) void lap_psi_kernel(const double *y, const double *a, const double *da, const double *f,
                                                       const double *df, double step, long N, double *res) {
    __shared__ double sh[16];
    double q = 0.0, lp = 0.0, md = 0.0, ma = 0.0;
    for (long i = threadIdx.x; i < N; i += 1024) {
        const double ai = fma(step, da[i], a[i]), fi = fma(step, df[i], f[i]);
        q = fma(ai, fi, q);
        lp += gp_log_ndtr(y[i] * fi);
        md = fmax(md, fabs(da[i]));
        ma = fmax(ma, fabs(ai));
    }
    q = lap_block_sum(q, sh);
    lp = lap_block_sum(lp, sh);
    md = lap_block_max(md, sh);
    ma = lap_block_max(ma, sh);
    if (threadIdx.x == 0) {
        res[1] = -0.5 * q;
        res[2] = lp;
        res[0] = res[1] + lp;
        res[3] = md;
        res[4] = ma;
    }
}
void launch_lap_psi(hipStream_t s, const double *y, const double *a, const double *da, const double *f, const double *df, double step,
                    long N, double *res) {
    GP_LAUNCH(lap_psi_kernel, dim3(1), dim3(1024), 0, s, y, a, da, f, df, step, N, res);
}

// a += step da, f += step df
__global__ __launch_bounds__(256) void lap_accept_kernel(double *a, const double *da, double *f, const double *df, double step, long N) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    a[i] = fma(step, da[i], a[i]);
    f[i] = fma(step, df[i], f[i]);
}
void launch_lap_accept(hipStream_t s, double *a, const double *da, double *f, const double *df, double step, long N) {
    GP_LAUNCH(lap_accept_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, a, da, f, df, step, N);
}

// min and max of W over the N rows: res[0], res[1]
__global__ __launch_bounds__(1024) void lap_wrange_kernel(const double *W, long N, double *res) {
    __shared__ double sh[16];
    double mn = INFINITY, mx = 0.0;
    for (long i = threadIdx.x; i < N; i += 1024) {
        mn = fmin(mn, W[i]);
        mx = fmax(mx, W[i]);
    }
    mn = -lap_block_max(-mn, sh);
    mx = lap_block_max(mx, sh);
    if (threadIdx.x == 0) {
        res[0] = mn;
        res[1] = mx;
    }
}
void launch_lap_wrange(hipStream_t s, const double *W, long N, double *res) {
    GP_LAUNCH(lap_wrange_kernel, dim3(1), dim3(1024), 0, s, W, N, res);
}

// ---- the handle's state after the fit: the factor of K + W^-1 is diag(W^-1/2) L -------------------------------------------------
// rows of L (lower tiles of A) divided by sqrt W; the columns of the inverted diagonal tiles (row-major 128 x 128 each) times it
__global__ __launch_bounds__(256) void lap_scale_factor_kernel(double *A, long lda, double *invL, const double *sw, long N, long Npad) {
    const long j = ((long)blockIdx.x * 256 + threadIdx.x) * 2, i = blockIdx.y;
    if (j >= Npad || j / GP_TILE > i / GP_TILE) return;
    if (i < N) {
        const double r = 1.0 / sw[i];
        double2_t v = *(double2_t *)(A + i * lda + j);
        v[0] *= r;
        v[1] *= r;
        *(double2_t *)(A + i * lda + j) = v;
    }
    if (j / GP_TILE == i / GP_TILE) {
        double *t = invL + (i / GP_TILE) * (long)GP_TILE * GP_TILE + (i % GP_TILE) * (long)GP_TILE + (j % GP_TILE);
        if (j < N) t[0] *= sw[j];
        if (j + 1 < N) t[1] *= sw[j + 1];
    }
}
void launch_lap_scale_factor(hipStream_t s, double *A, long lda, double *invL, const double *sw, long N, long Npad) {
    GP_LAUNCH(lap_scale_factor_kernel, dim3((unsigned)((Npad / 2 + 255) / 256), (unsigned)Npad), dim3(256), 0, s, A, lda, invL, sw, N,
              Npad);
}

// z = L^T a for the lower factor L in A: z_j = sum_{i >= j} L[i, j] a_i.  The right-hand-side row the prediction entries read
// (mean = (L^-1 k*) . z = k* . a).  64 columns a workgroup, four row classes folded in a fixed order
__global__ __launch_bounds__(256) void lap_ltvec_kernel(const double *A, long lda, const double *a, long N, long Npad, double *z) {
    __shared__ double sh[4][64];
    const int c = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const long j = (long)blockIdx.x * 64 + c;
    double s = 0.0;
    if (j < N)
        for (long i = (long)blockIdx.x * 64 + rg; i < N; i += 4)
            if (i >= j) s = fma(A[i * lda + j], a[i], s);
    sh[rg][c] = s;
    __syncthreads();
    if (rg == 0) z[j] = ((sh[0][c] + sh[1][c]) + sh[2][c]) + sh[3][c];
}
void launch_lap_ltvec(hipStream_t s, const double *A, long lda, const double *a, long N, long Npad, double *z) {
    GP_LAUNCH(lap_ltvec_kernel, dim3((unsigned)(Npad / 64)), dim3(256), 0, s, A, lda, a, N, Npad, z);
}

// ---- the gradient's vectors ------------------------------------------------------------------------------------------------------
// s2_i = 1/2 Sigma_ii t_i with the posterior variance of f_i, Sigma_ii = (K - C^T C)_ii = (1 - R_ii / W_i) / W_i, R = (K + W^-1)^-1:
// no N^3 product for the diagonal.  Where W is tiny the difference loses digits that t / W ~ |z| gives back: absolute error of
// a few ulp of |z|
__global__ __launch_bounds__(256) void lap_s2_kernel(const double *R, long ldr, const double *W, const double *t, long N, long Npad,
                                                     double *s2) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= Npad) return;
    s2[i] = (i < N) ? 0.5 * (t[i] / W[i]) * (1.0 - R[i * ldr + i] / W[i]) : 0.0;
}
void launch_lap_s2(hipStream_t s, const double *R, long ldr, const double *W, const double *t, long N, long Npad, double *s2) {
    GP_LAUNCH(lap_s2_kernel, dim3((unsigned)((Npad + 255) / 256)), dim3(256), 0, s, R, ldr, W, t, N, Npad, s2);
}
