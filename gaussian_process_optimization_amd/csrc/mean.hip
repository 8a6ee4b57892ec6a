// The affine mean function m(x) = x^T A + b of the exact GP (GPy core/gp.py:89-95, 267-271, 293-294 over mappings/linear.py,
// mappings/constant.py, mappings/additive.py): the residuals the fit factors against, m(x*) under a table's posterior mean, A under
// its x-gradient, and the mapping's own LML gradient  dL/dA = X^T alpha,  dL/db = 1^T alpha  (Linear.update_gradients,
// linear.py:35-36; Constant.update_gradients).
//
// Ab is ONE device vector: A [D, P] row-major, then b [P]; an absent part is held as zeros.  m(x)_p is formed in one place
// (mean_at below, and the same chain in the rows finish pass, rows_body.h): it starts from b_p and takes the D products in
// dimension order by fma -- a function of the location and the parameters alone, so the same inputs give the same bits in every
// kernel, slot and launch geometry.
//
// Plain fp64 FMA, no MFMA: D multiply-adds per element against an N^3 factorisation beside it; every kernel here is bound by
// reading its operands once.
#include "gphip_internal.h"

__device__ __forceinline__ double mean_at(const double *x, int D, int P, int p, const double *Ab) {
    double s = Ab[(long)D * P + p];
    for (int d = 0; d < D; ++d) s = fma(x[d], Ab[(long)d * P + p], s);
    return s;
}

// R[i, p] = Y[i, p] - m(X_i)_p, i < N: what the fit reads while a mean is resident
__global__ __launch_bounds__(256) void mean_residual_kernel(const double *X, const double *Y, long N, int D, int P, const double *Ab,
                                                            double *R) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= N * P) return;
    const long i = e / P;
    const int p = (int)(e % P);
    R[e] = Y[e] - mean_at(X + i * D, D, P, p, Ab);
}
void launch_mean_residual(hipStream_t s, const double *X, const double *Y, long N, int D, int P, const double *Ab, double *R) {
    const long n = N * P;
    GP_LAUNCH(mean_residual_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, X, Y, N, D, P, Ab, R);
}

// mean[m, p] += m(Xs_m)_p, m < M: behind the posterior reduction of a table (or of one of its chunks)
__global__ __launch_bounds__(256) void mean_add_kernel(const double *Xs, long M, int D, int P, const double *Ab, double *mean) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= M * P) return;
    const long m = e / P;
    const int p = (int)(e % P);
    mean[e] += mean_at(Xs + m * D, D, P, p, Ab);
}
void launch_mean_add(hipStream_t s, const double *Xs, long M, int D, int P, const double *Ab, double *mean) {
    const long n = M * P;
    GP_LAUNCH(mean_add_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, Xs, M, D, P, Ab, mean);
}

// dmdx[m, d, p] += A[d, p], m < M
__global__ __launch_bounds__(256) void mean_add_grad_kernel(long M, int DP, const double *Ab, double *dmdx) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= M * DP) return;
    dmdx[e] += Ab[e % DP];
}
void launch_mean_add_grad(hipStream_t s, long M, int D, int P, const double *Ab, double *dmdx) {
    const long n = M * (long)D * P;
    GP_LAUNCH(mean_add_grad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, M, D * P, Ab, dmdx);
}

// ---- dL/dA = X^T alpha [D, P], dL/db = 1^T alpha [P] ----------------------------------------------------------------------------
// Two levels over N, the order fixed by MEAN_GRAD_CH alone: workgroup c adds the terms of rows [c CH, (c + 1) CH) from 0 in row
// order, one thread per output element (d, p) -- row D of the outputs is db, its "input" the constant 1 --, and writes
// part[c][(D + 1) P]; mean_grad_combine_kernel adds the chunks' partials in chunk order, one thread per element.  One writer per
// partial, no atomics.
__global__ __launch_bounds__(256) void mean_grad_chunk_kernel(const double *X, const double *alpha, long ldal, long N, int D, int P,
                                                              double *part) {
    const int nout = (D + 1) * P;
    const long i0 = (long)blockIdx.x * MEAN_GRAD_CH, i1 = min(i0 + MEAN_GRAD_CH, N);
    for (int o = threadIdx.x; o < nout; o += 256) {
        const int d = o / P, p = o % P;
        const double *al = alpha + (long)p * ldal;
        double s = 0.0;
        if (d < D)
            for (long i = i0; i < i1; ++i) s = fma(X[i * D + d], al[i], s);
        else
            for (long i = i0; i < i1; ++i) s += al[i];
        part[(long)blockIdx.x * nout + o] = s;
    }
}
__global__ __launch_bounds__(256) void mean_grad_combine_kernel(const double *part, int nch, int nout, double *out) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= nout) return;
    double s = 0.0;
    for (int c = 0; c < nch; ++c) s += part[(long)c * nout + o];
    out[o] = s;
}
int mean_grad_chunks(long N) { return (int)((N + MEAN_GRAD_CH - 1) / MEAN_GRAD_CH); }
void launch_mean_grad(hipStream_t s, const double *X, const double *alpha, long ldal, long N, int D, int P, double *part, double *out) {
    const int nch = mean_grad_chunks(N), nout = (D + 1) * P;
    GP_LAUNCH(mean_grad_chunk_kernel, dim3((unsigned)nch), dim3(256), 0, s, X, alpha, ldal, N, D, P, part);
    GP_LAUNCH(mean_grad_combine_kernel, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, s, part, nch, nout, out);
}
