// The one-location passes over an ENSEMBLE: S hyper-parameter members over the context's (X, Y), each with an explicit inverse
// factor, alpha, parameters and fmin of its own (gp_ens_fit, api_ens.hip), answered in the launches of ONE model's call.
//
// The reference's MCMC model writes every HMC sample into the model and refactorises for every acquisition call
// (GPyOpt/GPyOpt/models/gpmodel.py:266-272 predict, :307-315 predict_withGradients, :285-291 get_fmin), and the integrated
// acquisitions average the per-sample rule (acquisitions/EI_mcmc.py:32-59, MPI_mcmc.py:32-59, LCB_mcmc.py:33-60).  Here the S
// posteriors stay resident and the member is a grid dimension (blockIdx.y) of the three passes of onerow.hip:
//
//   ens_forward_kernel    w_z = Li_z k*_z     k*_z generated in LDS from member z's own parameters
//   ens_backward_kernel   beta_z = Li_z^T w_z
//   ens_finish_kernel     member z's mean, variance, gradients and rule, written by the LAST workgroup of member z to arrive
//                         (one arrival counter per member); that workgroup then arrives at the ensemble's counter, and the
//                         last MEMBER to arrive averages the rule over the members in member order and writes the pinned
//                         result block with the pass's ticket behind it.
//
// The bodies are rows_body.h's -- what the single model's kernels run -- so member z's posterior is, bit for bit, what
// gp_predict_rows returns on a context fitted with z's parameters: whatever S, z's position and the locations that share the
// call.  No workgroup waits on another, every partial sum has one writer, every sum a fixed order: bitwise repeatable.
// The matrices are small (Npad <= 2048, the batched fit's cap): 32-row blocks, plain loads, four locations per pass.
#include "rows_body.h"

template <int MV>
__global__ __launch_bounds__(256) void ens_forward_kernel(EnsRows t, RowsX rx, const double *X, long N, long Npad, int nt) {
    const long z = blockIdx.y;
    rows_forward_body<MV, ENS_ROWS_RB, false>(blockIdx.x, t.Li + z * t.sLi, Npad, rx, t.kpt[z], X, N, t.alpha + z * t.sAlpha,
                                              t.wpart + z * t.sW, Npad, nt, t.meanpart + z * t.sM);
}

template <int MV>
__global__ __launch_bounds__(256) void ens_backward_kernel(EnsRows t, int M, long Npad) {
    const long z = blockIdx.y;
    rows_backward_body<MV, ENS_ROWS_RB, false>(blockIdx.x, t.Li + z * t.sLi, Npad, t.wpart + z * t.sW, Npad, M, t.bpart + z * t.sB,
                                               t.vpart + z * t.sV);
}

// post (device, per member, ENS_POST_STRIDE apart): the result block of rows_finish_body, laid out for MV locations
// out (host-visible): the integrated acquisition at [2 MV + m] and its gradient at [3 MV + 2 MV D + m D + d] -- where the single
// model's block carries them -- and the ticket at [ROWS_OUT_DOUBLES]
template <int MV>
__global__ __launch_bounds__(256) void ens_finish_kernel(EnsRows t, RowsX rx, const double *X, long N, long Npad, int nt, int want_grad,
                                                         int include_noise, int acq_on, int type, double par, int S,
                                                         unsigned int member_base, unsigned int ens_base, double *out, double ticket) {
    __shared__ int ens_last_s;
    const long z = blockIdx.y;
    const KernParams &kp = t.kpt[z];
    // no normaliser (the reference's MCMC model has none): y_mean = 0, y_std = 1; the member's own fmin
    const RowsAcq aq{acq_on, type, par, t.fmin[z], 0.0, 1.0, 0, 0, 0, nullptr, nullptr, nullptr};
    double *post = t.post + z * ENS_POST_STRIDE;
    if (!rows_finish_body<MV>(blockIdx.x, gridDim.x, rx, kp, X, N, t.alpha + z * t.sAlpha, t.wpart + z * t.sW, t.bpart + z * t.sB,
                              t.meanpart + z * t.sM, t.vpart + z * t.sV, Npad, nt, ENS_ROWS_RB, want_grad, kp.variance,
                              include_noise ? t.noise[z] : 0.0, aq, t.gpart + z * t.sG, t.counter + 1 + z, member_base, post))
        return;
    // member z is complete: its block is published, then the member arrives at the ensemble's counter
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) ens_last_s = (atomicAdd(t.counter, 1u) - ens_base == (unsigned)S - 1) ? 1 : 0;
    __syncthreads();
    if (!ens_last_s) return;
    __threadfence();
    if (acq_on) {
        const int D = kp.D, M = rx.M;
        const int nval = M * (1 + (want_grad ? D : 0));
        for (int v = threadIdx.x; v < nval; v += 256) {
            // v < M: the value of location v; beyond: gradient entry (m, d)
            const long src = v < M ? 2 * MV + v : 3 * MV + 2L * MV * D + (v - M);
            double s = 0.0;
            for (int k = 0; k < S; ++k) s += t.post[(long)k * ENS_POST_STRIDE + src];   // member order
            out[src] = s / (double)S;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) out[ROWS_OUT_DOUBLES] = ticket;
}

template <int MV>
static void launch_ens_rows_t(hipStream_t s, const EnsRows &t, int S, const RowsX &rx, const double *X, long N, long Npad, int want_grad,
                              int include_noise, int acq_on, int type, double par, const PassReport &r) {
    const int nt = (int)(Npad / GP_TILE);
    const dim3 tiles((unsigned)rows_tiles(nt) * (GP_TILE / ENS_ROWS_RB), (unsigned)S);
    const dim3 fin(rows_finish_grid(N), (unsigned)S);
    GP_LAUNCH(ens_forward_kernel<MV>, tiles, dim3(256), 0, s, t, rx, X, N, Npad, nt);
    if (want_grad) GP_LAUNCH(ens_backward_kernel<MV>, tiles, dim3(256), 0, s, t, rx.M, Npad);
    GP_LAUNCH(ens_finish_kernel<MV>, fin, dim3(256), 0, s, t, rx, X, N, Npad, nt, want_grad, include_noise, acq_on, type, par, S, r.base,
              r.base2, r.out, r.ticket);
}

void launch_ens_rows(hipStream_t s, const EnsRows &t, int S, const RowsX &rx, const double *X, long N, long Npad, int want_grad,
                     int include_noise, int acq_on, int type, double par, const PassReport &r) {
    if (rx.M == 1)
        launch_ens_rows_t<1>(s, t, S, rx, X, N, Npad, want_grad, include_noise, acq_on, type, par, r);
    else
        launch_ens_rows_t<ROWS_MAX_M>(s, t, S, rx, X, N, Npad, want_grad, include_noise, acq_on, type, par, r);
}

// ---- the table route's reduce: one workgroup per candidate row c --------------------------------------------------------------------
// Kx [S][ldr rows][Npad]: K_z(Xs, X) per member;  W [S][ldr][Npad]: Kx_z Li_z^T (the batched GEMM).  Per member: mean = Kx alpha,
// var = variance - |W|^2 + noise, the rule with the member's fmin; then the mean over members in member order.  The row sums
// run over i < N in a fixed order (thread stride, wave tree, waves in order).
__global__ __launch_bounds__(256) void ens_table_reduce_kernel(const double *Kx, const double *W, long ldr, long Npad, long N,
                                                               const double *alpha, long sAlpha, const KernParams *kpt,
                                                               const double *noise, const double *fmin, int S, int type, double par,
                                                               long M, double *out) {
    __shared__ double red[4];
    const long c = blockIdx.x;
    if (c >= M) return;
    double total = 0.0;
    for (int z = 0; z < S; ++z) {
        const double *kx = Kx + ((long)z * ldr + c) * Npad, *w = W + ((long)z * ldr + c) * Npad, *a = alpha + (long)z * sAlpha;
        double sm = 0.0, sv = 0.0;
        for (long i = threadIdx.x; i < N; i += 256) {
            sm = fma(kx[i], a[i], sm);
            sv = fma(w[i], w[i], sv);
        }
        const double mean = rw_block_sum(sm, red);
        const double ssq = rw_block_sum(sv, red);
        const double var = (kpt[z].variance - ssq) + noise[z];
        double f, c_m, c_s, ds_scale;
        acq_terms(type, par, fmin[z], 0.0, 1.0, mean, var, f, c_m, c_s, ds_scale);
        total += -f;
    }
    if (threadIdx.x == 0) out[c] = total / (double)S;
}

void launch_ens_table_reduce(hipStream_t s, const double *Kx, const double *W, long ldr, long Npad, long N, const double *alpha,
                             long sAlpha, const KernParams *kpt, const double *noise, const double *fmin, int S, int type, double par,
                             long M, double *out) {
    GP_LAUNCH(ens_table_reduce_kernel, dim3((unsigned)M), dim3(256), 0, s, Kx, W, ldr, Npad, N, alpha, sAlpha, kpt, noise, fmin, S, type,
              par, M, out);
}
