// Black-box constraints (Gardner et al. 2014; Gelbart et al. 2014): the probability of feasibility F(x) = prod_k Phi(z_k(x)) of K
// constraint GPs and the product it puts behind EI / MPI,  a_c = a F.  Everything is carried as log F = sum_k log Phi(z_k)
// (feas_terms, acq_math.h), summed in index order k = 0 .. K-1 in every kernel here: a location's bits do not depend on the route.
// Plain wave64 code: one thread per table row, or one workgroup of one wave per location with the dimensions dealt over its lanes.
#include "acq_math.h"

// logF[i] (+)= log Phi_k over the rows [0, M) of a constraint handle's table posterior (first: the sum starts here)
__global__ void feas_table_kernel(const double *mean, const double *var, long M, double c_mean, double c_std, double b, int first,
                                  double *logF) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    double t, lam, z, s;
    feas_terms(mean[i], var[i], c_mean, c_std, b, t, lam, z, s);
    logF[i] = first ? t : logF[i] + t;
}
void launch_feas_table(hipStream_t s, const double *mean, const double *var, long M, double c_mean, double c_std, double b,
                       int first, double *logF) {
    if (M <= 0) return;
    GP_LAUNCH(feas_table_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, mean, var, M, c_mean, c_std, b, first, logF);
}

// acq[i] <- acq[i] exp(logF[i]) over a table of negated scores; pof: the rule whose value is 1 (negated: -1) takes acq's place
__global__ void feas_apply_kernel(const double *logF, long M, int pof, double *acq) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const double old = pof ? -1.0 : acq[i];
    acq[i] = old * exp(logF[i]);
}
void launch_feas_apply(hipStream_t s, const double *logF, long M, int pof, double *acq) {
    if (M <= 0) return;
    GP_LAUNCH(feas_apply_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, logF, M, pof, acq);
}

// One workgroup (one wave) per location m < M: every lane forms the K terms -- the same instructions on the same operands, no
// divergence --, lane 0 keeps the value, the dimensions are dealt over the lanes.  neg given: neg <- neg F, dneg <- F (dneg +
// neg dlogF) in place, F = exp(logF) (pof: neg = -1, dneg = 0 come in).  neg null: logF [M] and (grad) dlogF [M, D] are written.
__global__ __launch_bounds__(64) void feas_rows_kernel(FeasRows fr, int M, int D, int grad, int pof, double *neg, double *dneg,
                                                       double *logF, double *dlogF) {
    const int m = blockIdx.x, tid = threadIdx.x;
    if (m >= M) return;
    double lam[FEAS_MAX_K], z[FEAS_MAX_K], s[FEAS_MAX_K];
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < FEAS_MAX_K; ++k) {
        if (k < fr.K) {
            double t;
            feas_terms(fr.mean[k][m], fr.var[k][m], fr.c_mean[k], fr.c_std[k], fr.bound[k], t, lam[k], z[k], s[k]);
            acc = k == 0 ? t : acc + t;
        }
    }
    const double F = exp(acc);
    const double old = neg ? (pof ? -1.0 : neg[m]) : 0.0;
    if (grad) {
        for (int d = tid; d < D; d += 64) {
            double gs = 0.0;
#pragma unroll
            for (int k = 0; k < FEAS_MAX_K; ++k) {
                if (k < fr.K) {
                    const double gk = feas_grad(lam[k], z[k], s[k], fr.c_std[k], fr.dm[k][(long)m * D + d], fr.dv[k][(long)m * D + d]);
                    gs = k == 0 ? gk : gs + gk;
                }
            }
            if (neg) {
                const double dold = pof ? 0.0 : dneg[(long)m * D + d];
                dneg[(long)m * D + d] = F * (dold + old * gs);
            } else {
                dlogF[(long)m * D + d] = gs;
            }
        }
    }
    __syncthreads();   // every lane has read neg[m]
    if (tid == 0) {
        if (neg) neg[m] = old * F;
        else logF[m] = acc;
    }
}
void launch_feas_rows(hipStream_t s, const FeasRows &fr, int M, int D, int grad, int pof, double *neg, double *dneg, double *logF,
                      double *dlogF) {
    if (M <= 0) return;
    GP_LAUNCH(feas_rows_kernel, dim3((unsigned)M), dim3(64), 0, s, fr, M, D, grad, pof, neg, dneg, logF, dlogF);
}

// out[i] = v[rows[i]] for i < n (gp_fmin_rows: the listed training rows' values, ahead of the arg-best reduction)
__global__ void feas_gather_kernel(const double *v, const long long *rows, long n, double *out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = v[rows[i]];
}
void launch_feas_gather(hipStream_t s, const double *v, const long long *rows, long n, double *out) {
    if (n <= 0) return;
    GP_LAUNCH(feas_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, v, rows, n, out);
}
