// Expected hypervolume improvement (Emmerich et al. 2011; Yang et al. 2019) of K = 2 or 3 independent objective GPs, all minimised:
//   EHVI(x) = sum_c prod_k D_ck,   D_ck = Psi_k(u_ck) - Psi_k(l_ck)   (ehvi_level, acq_math.h)
// over the C cells of the region the observed Pareto front does not dominate, and for the gradient the 2 K partials
//   G_mk = sum_c (prod_{j != k} D_cj) (Phi_k(l_ck) - Phi_k(u_ck)),   G_sk = sum_c (prod_{j != k} D_cj) (phi_k(u_ck) - phi_k(l_ck)),
//   d EHVI / dx_d = sum_k G_mk y_std_k dmdx_k[d] + G_sk y_std_k^2 dvdx_k[d] / (2 s_k).
// A cell's corners are indices into K sorted level arrays, so Psi, Phi, phi are evaluated once per level, not once per cell.
// ONE device routine serves a location, whichever kernel brings it: its bits do not depend on the route or on its company, and the
// value does not depend on whether the gradient is asked for.  Plain wave64 fp64 code, no atomics, nothing contracted into an fma.
#include "acq_math.h"

#define EHVI_WAVES (EHVI_THREADS / 64)
#define EHVI_NRED (1 + 2 * EHVI_MAX_K)   // what the threads' sums are: the value, G_m [K], G_s [K]

// Location m, by the whole workgroup of EHVI_THREADS threads.
//   1  the threads fill the LDS table of Psi (with grad: Phi and phi as well) for the K L levels;
//   2  thread t takes cells t, t + EHVI_THREADS, ... in increasing order;
//   3  the threads' sums meet in a tree over the 64 lanes of each wave (lane i takes lane i + 32, + 16, ... + 1), then the waves'
//      sums are added in wave order;
//   4  the dimensions are dealt over the threads.
// neg[m] <- -EHVI, dneg[m D + d] <- -d EHVI / dx_d.
__device__ __forceinline__ void ehvi_location(const EhviCells &ec, const EhviRows &er, long m, int D, int grad, double *neg,
                                              double *dneg) {
#pragma clang fp contract(off)
    __shared__ double sPsi[EHVI_MAX_K * EHVI_MAX_L], sPhi[EHVI_MAX_K * EHVI_MAX_L], sphi[EHVI_MAX_K * EHVI_MAX_L];
    __shared__ double sS[EHVI_MAX_K], sRed[EHVI_WAVES * EHVI_NRED], sTot[EHVI_NRED];
    const int tid = threadIdx.x, K = ec.K;
#pragma unroll
    for (int k = 0; k < EHVI_MAX_K; ++k) {
        if (k < K) {
            const double mean = er.mean[k][m], var = er.var[k][m];
            for (int i = tid; i < ec.L[k]; i += EHVI_THREADS) {
                double Psi, Phi, phi, s;
                ehvi_level(mean, var, er.y_mean[k], er.y_std[k], ec.levels[ec.off[k] + i], Psi, Phi, phi, s);
                sPsi[ec.off[k] + i] = Psi;
                if (grad) {
                    sPhi[ec.off[k] + i] = Phi;
                    sphi[ec.off[k] + i] = phi;
                }
                if (i == 0) sS[k] = s;
            }
        }
    }
    __syncthreads();
    double r[EHVI_NRED];
#pragma unroll
    for (int j = 0; j < EHVI_NRED; ++j) r[j] = 0.0;
    for (int c = tid; c < ec.C; c += EHVI_THREADS) {
        double dl[EHVI_MAX_K], dP[EHVI_MAX_K], dp[EHVI_MAX_K];
#pragma unroll
        for (int k = 0; k < EHVI_MAX_K; ++k) {
            dl[k] = 1.0;
            dP[k] = dp[k] = 0.0;
            if (k < K) {
                const unsigned int w = ec.cells[(long)c * K + k];
                const int lo = ec.off[k] + (int)(w & 0xffffu), hi = ec.off[k] + (int)(w >> 16);
                dl[k] = sPsi[hi] - sPsi[lo];
                if (grad) {
                    dP[k] = sPhi[lo] - sPhi[hi];
                    dp[k] = sphi[hi] - sphi[lo];
                }
            }
        }
        const double d01 = dl[0] * dl[1];
        r[0] += K == 3 ? d01 * dl[2] : d01;
        if (grad) {
            const double o0 = K == 3 ? dl[1] * dl[2] : dl[1], o1 = K == 3 ? dl[0] * dl[2] : dl[0];
            r[1] += o0 * dP[0];
            r[2] += o1 * dP[1];
            r[1 + EHVI_MAX_K] += o0 * dp[0];
            r[2 + EHVI_MAX_K] += o1 * dp[1];
            if (K == 3) {
                r[3] += d01 * dP[2];
                r[3 + EHVI_MAX_K] += d01 * dp[2];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < EHVI_NRED; ++j) {
        if (j == 0 || grad) {
            double v = r[j];
            for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
            if ((tid & 63) == 0) sRed[(tid >> 6) * EHVI_NRED + j] = v;
        }
    }
    __syncthreads();
    if (tid < EHVI_NRED && (tid == 0 || grad)) {
        double v = sRed[tid];
        for (int w = 1; w < EHVI_WAVES; ++w) v += sRed[w * EHVI_NRED + tid];
        sTot[tid] = v;
    }
    __syncthreads();
    if (tid == 0) neg[m] = -sTot[0];
    if (!grad) return;
    for (int d = tid; d < D; d += EHVI_THREADS) {
        double g = 0.0;
#pragma unroll
        for (int k = 0; k < EHVI_MAX_K; ++k) {
            if (k < K) {
                const double ys = er.y_std[k];
                const double t = (sTot[1 + k] * ys) * er.dm[k][m * D + d] +
                                 ((sTot[1 + EHVI_MAX_K + k] * (ys * ys)) * er.dv[k][m * D + d]) / (2.0 * sS[k]);
                g = k == 0 ? t : g + t;
            }
        }
        dneg[m * D + d] = -g;
    }
}

__global__ __launch_bounds__(EHVI_THREADS) void ehvi_table_kernel(EhviCells ec, EhviRows er, long M, double *neg) {
    const long m = blockIdx.x;
    if (m >= M) return;
    ehvi_location(ec, er, m, 0, 0, neg, nullptr);
}
void launch_ehvi_table(hipStream_t s, const EhviCells &ec, const EhviRows &er, long M, double *neg) {
    if (M <= 0) return;
    GP_LAUNCH(ehvi_table_kernel, dim3((unsigned)M), dim3(EHVI_THREADS), 0, s, ec, er, M, neg);
}

__global__ __launch_bounds__(EHVI_THREADS) void ehvi_rows_kernel(EhviCells ec, EhviRows er, int M, int D, int grad, double *neg,
                                                                 double *dneg) {
    const int m = blockIdx.x;
    if (m >= M) return;
    ehvi_location(ec, er, m, D, grad, neg, dneg);
}
void launch_ehvi_rows(hipStream_t s, const EhviCells &ec, const EhviRows &er, int M, int D, int grad, double *neg, double *dneg) {
    if (M <= 0) return;
    GP_LAUNCH(ehvi_rows_kernel, dim3((unsigned)M), dim3(EHVI_THREADS), 0, s, ec, er, M, D, grad, neg, dneg);
}
