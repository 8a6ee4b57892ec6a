// The joint (batch) expected improvement of q <= 8 locations, by Monte Carlo over fixed base samples (sample-average approximation):
//     qEI(x_1 .. x_q) = (1 / S) sum_s max(0, max_j (fmin - par - y_sj)),    y_s = m + C z_s,   C C^T = Sigma,
// m and Sigma the JOINT posterior of the q locations (Ginsbourger et al. 2010; Wang et al. 2016; Wilson et al. 2018 for the
// reparameterised gradient).  With the base samples z_s fixed the estimate is a deterministic, piecewise smooth function of the
// q D coordinates, which L-BFGS-B can take.
//
// The N^2 work is the fused rows path's own (onerow.hip): ONE forward pass over the inverse factor gives w_i = Li k_i for all q
// locations, and a gradient call ONE backward pass beta_i = Li^T w_i.  Three kernels are new:
//
//   qei_gram_kernel    w_i . w_j for j <= i: per 64 training rows one partial, formed and later added exactly as the finishing kernel of
//                      a value call forms |w_i|^2 -- the diagonal is that sum, bit for bit
//   qei_joint_kernel   one workgroup: m, Sigma = k(x_i, x_j) - w_i . w_j (+ noise on the diagonal), de-normalised; C = chol(Sigma) in every
//                      thread's registers; the S samples, thread t taking s = t, t + 256, ... in order; the adjoint mbar, Cbar -> Sigma_bar = sym(C^-T tril*(C^T
//                      Cbar) C^-1) (Murray 2016, the Cholesky's reverse mode); A = 2 Sigma_bar
//   qei_close_kernel   over the training points: d qEI / d x_i = mbar_i J_i^T alpha - J_i^T (sum_j A_ij beta_j) + sum_j A_ij dk(x_i, x_j)/dx_i,
//                      J_i the input Jacobian of k(X, x_i) -- the finishing kernel's gradients_X sums with t_i = sum_j A_ij beta_j in the
//                      place of -2 beta_i: the q x q adjoint is mixed in AFTER the backward pass, which therefore stays one pass
//
// Every sum has one writer per partial and a fixed order that does not depend on the grid: no atomics but the arrival counter.
#include "rows_body.h"

__device__ __forceinline__ void qei_pair(int p, int &i, int &j) {   // p = i (i + 1) / 2 + j, j <= i
    i = 0;
    while ((i + 1) * (i + 2) / 2 <= p) ++i;
    j = p - i * (i + 1) / 2;
}

// ---- Gram of the w_i ----------------------------------------------------------------------------------------------------------------------
// grid = rows_finish_grid(N) workgroups of 256 threads, 64 training rows each: w_m[n] = sum_C wpart[C][m][n] split between the four waves
// and added in wave order (rows_finish_body's value call), then one wave sum per pair.  gpart row: M (M + 1) / 2 sums, RW_GROW apart.
__global__ __launch_bounds__(256) void qei_gram_kernel(const double *wpart, long Npad, long N, int M, int MV, double *gpart) {
    __shared__ double part_s[4][ROWS_WIDE_M][64];
    __shared__ double w_s[ROWS_WIDE_M][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long n = (long)blockIdx.x * 64 + lane;
    const bool live = n < N;
    const int Rn = (int)(n / GP_TILE);
    for (int m = 0; m < M; ++m) {
        double s = 0.0;
        if (live) s = rw_strided_sum(wpart + (long)m * Npad + n, (long)MV * Npad, wave, 4, rw_nch(Rn));
        part_s[wave][m][lane] = s;
    }
    __syncthreads();
    for (int i = tid; i < M * 64; i += 256) {
        const int m = i >> 6, l = i & 63;
        w_s[m][l] = ((part_s[0][m][l] + part_s[1][m][l]) + part_s[2][m][l]) + part_s[3][m][l];
    }
    __syncthreads();
    const int npair = M * (M + 1) / 2;
    for (int p = wave; p < npair; p += 4) {
        int i, j;
        qei_pair(p, i, j);
        const double a = w_s[i][lane], b = w_s[j][lane];
        const double v = rw_wave_sum(a * b);
        if (lane == 0) gpart[(long)blockIdx.x * RW_GROW + p] = v;
    }
}

void launch_qei_gram(hipStream_t s, int M, long N, long Npad, const RowsWork &w) {
    GP_LAUNCH(qei_gram_kernel, dim3(rows_finish_grid(N)), dim3(256), 0, s, w.wpart, Npad, N, M, rows_layout(M), w.gpart);
}

// ---- the joint step -------------------------------------------------------------------------------------------------------------------------
#define QEI_NPAIR (ROWS_WIDE_M * (ROWS_WIDE_M + 1) / 2)
#define QEI_NSUM (1 + ROWS_WIDE_M + QEI_NPAIR)   // the value, the counts, the lower triangle of Cbar
__global__ __launch_bounds__(256) void qei_joint_kernel(RowsX rx, KernParams kp, const double *gpart, int nblk, const double *meanpart,
                                                        int nmean, int MV, double kss, double noise_add, QeiArgs qa, int want_grad,
                                                        double *state, double *out, double ticket) {
    constexpr int Q = ROWS_WIDE_M;
    __shared__ double xs_s[ROWS_MAX_XS];
    __shared__ double fin_s[8][QEI_NPAIR + Q];
    __shared__ double res_s[QEI_NPAIR + Q];
    __shared__ double m_s[Q], Sig_s[Q][Q], C_s[Q][Q];
    __shared__ double cnt_s[Q], Cb_s[Q][Q], P_s[Q][Q], U_s[Q][Q], T_s[Q][Q];
    __shared__ double part_s[256][QEI_NSUM];   // (an odd stride: the threads' rows fall on different banks)
    __shared__ double gsum_s[4][QEI_NSUM];
    __shared__ double val_s;
    const int tid = threadIdx.x;
    const int D = kp.D, M = rx.M;
    const int npair = M * (M + 1) / 2, ntot = npair + M;
    for (int i = tid; i < M * D; i += 256) xs_s[i] = rx.xs[i] / kp.ls[i % D];
    // the workgroups' Gram partials and the chunks' mean terms, each in eight interleaved slices added in slice order (rows_finish_body)
    for (int idx = tid; idx < 8 * ntot; idx += 256) {
        const int v = idx % ntot, j = idx / ntot;
        fin_s[j][v] = v < npair ? rw_strided_sum(gpart + v, RW_GROW, j, 8, nblk) : rw_strided_sum(meanpart + (v - npair), MV, j, 8, nmean);
    }
    __syncthreads();
    for (int v = tid; v < ntot; v += 256) {
        double s = 0.0;
        for (int j = 0; j < 8; ++j) s += fin_s[j][v];
        res_s[v] = s;
    }
    __syncthreads();
    const double ys2 = qa.y_std * qa.y_std;
    if (tid < Q * Q) {
        const int i = tid / Q, j = tid % Q;
        if (i < M && j <= i) {
            double v;
            if (i == j) {
                v = (kss - res_s[i * (i + 1) / 2 + i]) + noise_add;   // the finishing kernel's variance
            } else {
                double r2 = 0.0;
                for (int d = 0; d < D; ++d) {
                    const double df = xs_s[i * D + d] - xs_s[j * D + d];
                    r2 = fma(df, df, r2);
                }
                v = gp_k_of_r2(kp.kernel, kp.variance, r2) - res_s[i * (i + 1) / 2 + j];
            }
            v *= ys2;
            Sig_s[i][j] = v;
            Sig_s[j][i] = v;
        }
        if (i < M && j == 0) m_s[i] = res_s[npair + i] * qa.y_std + qa.y_mean;
    }
    __syncthreads();
    // C = chol(Sigma), lower, rows in the caller's order.  EVERY thread factors the same matrix in registers, left-looking (one thread
    // alone would take as long, and the factor would have to travel through LDS to the samples' loop); a pivot is the same in all
    // of them, so the exit below is uniform.
#define QEI_P(i, l) ((i) * ((i) + 1) / 2 + (l))
    double Cr[QEI_NPAIR], mr[Q];
#pragma unroll
    for (int p = 0; p < QEI_NPAIR; ++p) Cr[p] = 0.0;
    int bad = 0;
#pragma unroll
    for (int j = 0; j < Q; ++j) {
        mr[j] = j < M ? m_s[j] : 0.0;
        if (j < M && !bad) {
            double piv = Sig_s[j][j];
#pragma unroll
            for (int l = 0; l < j; ++l) piv -= Cr[QEI_P(j, l)] * Cr[QEI_P(j, l)];
            if (!(piv > 0.0) || !isfinite(piv)) bad = j + 1;
            const double c = sqrt(piv);
            Cr[QEI_P(j, j)] = c;
#pragma unroll
            for (int i = j + 1; i < Q; ++i) {
                if (i < M) {
                    double v = Sig_s[i][j];
#pragma unroll
                    for (int l = 0; l < j; ++l) v -= Cr[QEI_P(i, l)] * Cr[QEI_P(j, l)];
                    Cr[QEI_P(i, j)] = v / c;
                }
            }
        }
    }
    if (bad) {
        if (tid == 0) {
            state[0] = (double)bad;
            out[QEI_OUT_STATUS] = (double)bad;
            if (!want_grad) out[ROWS_OUT_DOUBLES] = ticket;
        }
        return;
    }
    if (tid == 0) {   // ... and to LDS for the adjoint's substitutions, zeros above the diagonal and beyond M
#pragma unroll
        for (int i = 0; i < Q; ++i)
#pragma unroll
            for (int l = 0; l < Q; ++l) C_s[i][l] = l <= i ? Cr[QEI_P(i, l)] : 0.0;
    }
    // the samples: thread t takes s = t, t + 256, ... in order (Z lies column-major: a wave's loads of one column are one line each,
    // and the next sample's are issued ahead of this one's arithmetic)
    double val = 0.0, cnt[Q], cb[QEI_NPAIR], zn[Q];
#pragma unroll
    for (int j = 0; j < Q; ++j) cnt[j] = 0.0;
#pragma unroll
    for (int p = 0; p < QEI_NPAIR; ++p) cb[p] = 0.0;
    const double t0 = qa.fmin - qa.par;
#pragma unroll
    for (int l = 0; l < Q; ++l) zn[l] = (l < M && tid < qa.S) ? qa.Z[(long)l * qa.ldz + tid] : 0.0;
    for (int s = tid; s < qa.S; s += 256) {
        double z[Q];
#pragma unroll
        for (int l = 0; l < Q; ++l) {
            z[l] = zn[l];
            zn[l] = (l < M && s + 256 < qa.S) ? qa.Z[(long)l * qa.ldz + s + 256] : 0.0;
        }
        double best = -INFINITY;
        int jst = 0;
#pragma unroll
        for (int j = 0; j < Q; ++j) {
            if (j < M) {
                double y = mr[j];
#pragma unroll
                for (int l = 0; l <= j; ++l) y = fma(Cr[QEI_P(j, l)], z[l], y);
                const double I = t0 - y;
                if (I > best) {   // the lowest j on a tie
                    best = I;
                    jst = j;
                }
            }
        }
        const bool active = best > 0.0;
        val += active ? best : 0.0;
#pragma unroll
        for (int j = 0; j < Q; ++j) {
            const bool sel = active && jst == j;
            cnt[j] += sel ? 1.0 : 0.0;
#pragma unroll
            for (int l = 0; l <= j; ++l) cb[QEI_P(j, l)] += sel ? z[l] : 0.0;
        }
    }
    // The threads' 1 + M + M (M + 1) / 2 sums through LDS: thread (e, g) adds entry e of the threads 64 g .. 64 g + 63 in thread
    // order, then the four groups are added in order.  (A shuffle tree per entry took 0.4 us apiece, 17 us at q = 8.)
    const int ne = 1 + M + npair;
    part_s[tid][0] = val;
#pragma unroll
    for (int j = 0; j < Q; ++j) {
        if (j < M) {
            part_s[tid][1 + j] = cnt[j];
#pragma unroll
            for (int l = 0; l <= j; ++l) part_s[tid][1 + M + QEI_P(j, l)] = cb[QEI_P(j, l)];
        }
    }
    __syncthreads();
    if (tid < 4 * ne) {
        const int e = tid % ne, g = tid / ne;
        double sum = 0.0;
        for (int i = 0; i < 64; ++i) sum += part_s[g * 64 + i][e];
        gsum_s[g][e] = sum;
    }
    __syncthreads();
    if (tid < ne) {
        const double tot = ((gsum_s[0][tid] + gsum_s[1][tid]) + gsum_s[2][tid]) + gsum_s[3][tid];
        if (tid == 0) {
            val_s = tot;
        } else if (tid <= M) {
            cnt_s[tid - 1] = tot;
        } else {
            int j, l;
            qei_pair(tid - 1 - M, j, l);
            Cb_s[j][l] = tot;
        }
    }
    __syncthreads();
    const double inv_s = 1.0 / (double)qa.S;
    // P = tril(C^T Cbar), its diagonal halved (Cbar = -(1 / S) the sums, lower)
    if (tid < Q * Q) {
        const int a = tid / Q, b = tid % Q;
        double p = 0.0;
        if (a < M && b <= a) {
            for (int k = a; k < M; ++k) p = fma(C_s[k][a], -(Cb_s[k][b] * inv_s), p);
            if (a == b) p *= 0.5;
        }
        P_s[a][b] = p;
    }
    __syncthreads();
    // Sigma_bar = sym(C^-T P C^-1) by two back substitutions against the factor in registers: thread b column b of U = C^-T P, then
    // thread a row a of T = U C^-1 (entries beyond M are zeros of Cr and of P: they add nothing)
    {
        const int b = tid < M ? tid : 0;
        double u[Q];
#pragma unroll
        for (int a = Q - 1; a >= 0; --a) {
            double v = P_s[a][b];
#pragma unroll
            for (int k = a + 1; k < Q; ++k) v -= Cr[QEI_P(k, a)] * u[k];
            u[a] = a < M ? v / Cr[QEI_P(a, a)] : 0.0;
        }
        if (tid < M) {
#pragma unroll
            for (int a = 0; a < Q; ++a) U_s[a][b] = u[a];
        }
    }
    __syncthreads();
    {
        const int a = tid < M ? tid : 0;
        double t[Q];
#pragma unroll
        for (int b = Q - 1; b >= 0; --b) {
            double v = U_s[a][b];
#pragma unroll
            for (int k = b + 1; k < Q; ++k) v -= t[k] * Cr[QEI_P(k, b)];
            t[b] = b < M ? v / Cr[QEI_P(b, b)] : 0.0;
        }
        if (tid < M) {
#pragma unroll
            for (int b2 = 0; b2 < Q; ++b2) T_s[a][b2] = t[b2];
        }
    }
#undef QEI_P
    __syncthreads();
    // results; for the closing pass mbar and A = 2 sym(T) of the NORMALISED model (d m' = y_std d m, d Sigma' = y_std^2 d Sigma)
    if (tid < Q * Q) {
        const int i = tid / Q, j = tid % Q;
        if (i < M && j < M) {
            out[QEI_OUT_COV + i * M + j] = Sig_s[i][j];
            state[1 + Q + i * Q + j] = (T_s[i][j] + T_s[j][i]) * ys2;
        }
        if (i < M && j == 0) {
            out[QEI_OUT_MEAN + i] = m_s[i];
            state[1 + i] = -(cnt_s[i] * inv_s) * qa.y_std;
        }
    }
    if (tid == 0) {
        state[0] = 0.0;
        out[QEI_OUT_STATUS] = 0.0;
        out[QEI_OUT_VALUE] = -(val_s * inv_s);
    }
    __syncthreads();
    if (tid == 0 && !want_grad) out[ROWS_OUT_DOUBLES] = ticket;
}

void launch_qei_joint(hipStream_t s, const RowsX &rx, const KernParams &kp, long N, long Npad, const RowsWork &w, double kss,
                      double noise_add, const QeiArgs &qa, int want_grad, double *state, const PassReport &r) {
    const int nt = (int)(Npad / GP_TILE);
    GP_LAUNCH(qei_joint_kernel, dim3(1), dim3(256), 0, s, rx, kp, w.gpart, (int)rows_finish_grid(N), w.meanpart, rw_nch(nt - 1),
              rows_layout(rx.M), kss, noise_add, qa, want_grad, state, r.out, r.ticket);
}

// ---- the closing pass over the training points ----------------------------------------------------------------------------------------------
// grid = rows_finish_grid(N) workgroups of 256 threads, 64 training rows each (rows_finish_body's geometry): beta_j[n] from the backward
// pass's row-block partials, t_i[n] = sum_j A_ij beta_j[n] in index order, then location i (wave i % 4) takes row n through ONE
// gradients_X sum with the weight g (mbar_i alpha_n - t_i[n]).  The last workgroup to arrive adds the workgroups' sums in eight
// interleaved slices, the cross terms sum_j A_ij dk(x_i, x_j)/dx_i, and writes the NEGATED gradient and the ticket.
__global__ __launch_bounds__(256) void qei_close_kernel(RowsX rx, KernParams kp, const double *X, long N, const double *alpha,
                                                        const double *bpart, long Npad, int MV, int nt, int rbh, const double *state,
                                                        double *gpart, unsigned int *counter, unsigned int counter_base, double *out,
                                                        double ticket) {
    constexpr int Q = ROWS_WIDE_M;
    __shared__ double xs_s[ROWS_MAX_XS];
    __shared__ double part_s[4][Q][64];
    __shared__ double b_s[Q][64];
    __shared__ double A_s[Q][Q], mb_s[Q];
    __shared__ double fin_s[8][ROWS_MAX_XS];
    __shared__ double res_s[ROWS_MAX_XS];
    __shared__ int last_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int D = kp.D, M = rx.M;
    const bool ok = state[0] == 0.0;   // a failed factorisation: nothing to add up, the arrivals and the ticket alone
    const long n = (long)blockIdx.x * 64 + lane;
    const bool live = n < N;
    const int nrb = nt * (GP_TILE / rbh);
    if (ok) {
        for (int i = tid; i < M * D; i += 256) xs_s[i] = rx.xs[i] / kp.ls[i % D];
        if (tid < Q * Q) A_s[tid / Q][tid % Q] = state[1 + Q + tid];
        if (tid < Q) mb_s[tid] = state[1 + tid];
        for (int m = 0; m < M; ++m) {
            double s = 0.0;
            if (live) s = rw_strided_sum(bpart + (long)m * Npad + n, (long)MV * Npad, (int)(n / rbh) + wave, 4, nrb);
            part_s[wave][m][lane] = s;
        }
        __syncthreads();
        for (int i = tid; i < M * 64; i += 256) {
            const int m = i >> 6, l = i & 63;
            b_s[m][l] = ((part_s[0][m][l] + part_s[1][m][l]) + part_s[2][m][l]) + part_s[3][m][l];
        }
        __syncthreads();
        for (int i = wave; i < M; i += 4) {
            double t = 0.0;
            for (int j = 0; j < M; ++j) t = fma(A_s[i][j], b_s[j][lane], t);
            double s = 0.0, a = 0.0;
            if (live) {
                for (int d = 0; d < D; ++d) {
                    const double df = xs_s[i * D + d] - X[n * D + d] / kp.ls[d];
                    s = fma(df, df, s);
                }
                a = alpha[n];
            }
            double kv, gv;
            gp_k_and_g(kp.kernel, kp.variance, s, kv, gv);
            if (s == 0.0) gv = 0.0;   // invdist = 0 where the distance is exactly 0 (stationary.py:251-258)
            const double c = live ? gv * (mb_s[i] * a - t) : 0.0;
            for (int d = 0; d < D; ++d) {
                const double dq = live ? xs_s[i * D + d] - X[n * D + d] / kp.ls[d] : 0.0;
                const double v = rw_wave_sum(c * dq);
                if (lane == 0) gpart[(long)blockIdx.x * RW_GROW + i * D + d] = v;
            }
        }
    }
    __threadfence();
    __syncthreads();
    if (tid == 0) last_s = (atomicAdd(counter, 1u) - counter_base == gridDim.x - 1) ? 1 : 0;   // (unsigned: wraps with the base)
    __syncthreads();
    if (!last_s) return;
    __threadfence();
    if (ok) {
        const int nval = M * D;
        for (int idx = tid; idx < 8 * nval; idx += 256) {
            const int v = idx % nval, j = idx / nval;
            fin_s[j][v] = rw_strided_sum(gpart + v, RW_GROW, j, 8, (int)gridDim.x);
        }
        __syncthreads();
        for (int v = tid; v < nval; v += 256) {
            double s = 0.0;
            for (int j = 0; j < 8; ++j) s += fin_s[j][v];
            res_s[v] = s;
        }
        __syncthreads();
        for (int v = tid; v < nval; v += 256) {
            const int i = v / D, d = v % D;
            double cross = 0.0;   // sum_j A_ij g(r_ij) (x_i - x_j)_d / l_d, j in index order; j = i adds 0
            for (int j = 0; j < M; ++j) {
                if (j == i) continue;
                double r2 = 0.0;
                for (int e = 0; e < D; ++e) {
                    const double df = xs_s[i * D + e] - xs_s[j * D + e];
                    r2 = fma(df, df, r2);
                }
                double kv, gv;
                gp_k_and_g(kp.kernel, kp.variance, r2, kv, gv);
                if (r2 == 0.0) gv = 0.0;
                cross = fma(A_s[i][j] * gv, xs_s[i * D + d] - xs_s[j * D + d], cross);
            }
            out[QEI_OUT_GRAD + v] = -((res_s[v] + cross) / kp.ls[d]);   // (x - x') / l^2 = scaled difference / l
        }
        __syncthreads();
    }
    if (tid == 0) out[ROWS_OUT_DOUBLES] = ticket;
}

void launch_qei_close(hipStream_t s, const RowsX &rx, const KernParams &kp, const double *X, long N, long Npad, const double *alpha,
                      const RowsWork &w, const double *state, const PassReport &r) {
    const int nt = (int)(Npad / GP_TILE);
    GP_LAUNCH(qei_close_kernel, dim3(rows_finish_grid(N)), dim3(256), 0, s, rx, kp, X, N, alpha, w.bpart, Npad, rows_layout(rx.M), nt,
              rows_block_height(nt), state, w.gpart, r.counter, r.base, r.out, r.ticket);
}
