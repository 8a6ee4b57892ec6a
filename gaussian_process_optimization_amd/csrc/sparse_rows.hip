// The acquisition optimiser's one-location calls on the SPARSE model as ONE launch over woodbury_inv.
//
// scipy's L-BFGS-B evaluates the acquisition one location at a time, hundreds of times between two fits (see onerow.hip for the
// call chain).  Over a sparse model the reference needs per location x (posterior.py:225-248, gp.py:407-454 over
// _predictive_variable = Z)
//     k = K(x, Z),  mean = k . w,  b = woodbury_inv k,  var = max(kss - k . b, 1e-15) (+ noise),
//     d mean / dx = sum_j w_j dk_j/dx,  d var / dx = -2 sum_j b_j dk_j/dx
// and the EI / LCB / MPI (+ local penalisation) chain rule on top: matrix-vector work bound by ONE read of the Mz x Mz matrix
// (33.5 MB at the Mz = 2048 cap).  gp_sparse_predict does it as an upload, a cross-covariance launch, a 64 x 64-unit GEMM, a
// reduce, a gradient launch and four copies back; here it is
//
//   sparse_rows_kernel   a workgroup takes SPARSE_ROWS_RB rows of woodbury_inv.  Their first columns are requested at once (the loads
//                        do not depend on k and fly while it is formed); it generates k for every location of the pass into LDS
//                        (16 KB per location at the cap), forms b on its rows -- two rows per wave, all locations of the pass
//                        from one read of the rows --, then the rows' terms of k . b, k . w and of the two gradient sums.  The
//                        LAST workgroup to arrive adds the workgroups' sums in workgroup order and writes mean, variance,
//                        gradients, acquisition and penaliser straight into the caller-visible pinned block.
//
// The mean's gradient alone (estimate_L's inner call) needs only w: the same kernel in mode 2 skips k and the matrix.
// Locations travel in the kernel arguments and the results land in host-visible memory: no copy commands on either side of the
// launch.  Every partial sum has ONE writer and a fixed reduction order that does not depend on the number of locations or on a
// location's slot: the same bits whatever the company, on every call.
#include "gphip_internal.h"
#include "acq_math.h"

#define SR_MAXZ 2048      // GP_SPARSE_MAX_INDUCING (include/gphip.h): columns of k kept in LDS per location
#define SR_XS ROWS_MAX_XS
#define SR_GROW SPARSE_ROWS_GROW   // gpart row (per workgroup): [M D sums of d mean | at SR_XS: M D sums of d var | at 2 SR_XS: M of k . b | M of k . w]

__device__ __forceinline__ double sr_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}
// sum of p[i stride] for i = first, first + step, ... < end, added in that order; the loads go out eight at a time
__device__ __forceinline__ double sr_strided_sum(const double *p, long stride, int first, int step, int end) {
    double s = 0.0;
    for (int i = first; i < end; i += 8 * step) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int k = i + u * step;
            v[u] = k < end ? p[(long)k * stride] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
    }
    return s;
}

// mode 0: posterior (and acquisition) values; 1: values and gradients; 2: the mean's gradient alone.
// grid = sparse_rows_grid(Mz) workgroups of 256 threads; Winv is n x n row-major (n = Mz rounded up to the tile, at most SR_MAXZ).
// Zs [Mz, D] holds the inducing inputs already divided by the lengthscales, Z[j, d] / l_d (sparse_scale_z_kernel, at the first rows call after a fit): the
// quotients every covariance kernel forms on the fly, bit for bit, without 8 D divisions per thread and call.
// out (host-visible, laid out for ROWS_WIDE_M locations whatever M): [mean][var][acq][dmdx D][dvdx D][dacq D], then the ticket.
template <int MV>
__global__ __launch_bounds__(256) void sparse_rows_kernel(const double *Winv, long n, long Mz, RowsX rx, KernParams kp, const double *Zs,
                                                          const double *w, int mode, double kss, double noise_add, RowsAcq aq,
                                                          double *gpart, unsigned int *counter, unsigned int counter_base, double *out,
                                                          double ticket) {
    __shared__ __attribute__((aligned(16))) double ks[MV * SR_MAXZ];
    __shared__ double xs_s[SR_XS], xraw_s[SR_XS];
    __shared__ double bs[MV][SPARSE_ROWS_RB], gw[MV][SPARSE_ROWS_RB], gb[MV][SPARSE_ROWS_RB], kb[MV][SPARSE_ROWS_RB], kw[MV][SPARSE_ROWS_RB];
    __shared__ double fin_s[8][2 * SR_XS + 2 * MV];
    __shared__ double res_s[2 * SR_XS + 2 * MV];
    __shared__ double da_s[SR_XS];   // the acquisition's gradient while the penaliser works on it
    __shared__ int last_s;
    constexpr int RB = SPARSE_ROWS_RB;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int D = kp.D, M = rx.M;
    const long i0 = (long)blockIdx.x * RB;
    for (int i = tid; i < M * D; i += 256) {
        xraw_s[i] = rx.xs[i];
        xs_s[i] = rx.xs[i] / kp.ls[i % D];
    }
    __syncthreads();
    // this wave's two rows of Winv, r0 and r0 + 1 (r0 + 1 < n: the grid covers ceil(Mz / RB) RB <= n rows); a lane holds the column
    // pairs 2 lane + 128 q.  The first SR_PF of them are requested here, before k exists.
    constexpr int SR_PF = MV > ROWS_MAX_M ? 4 : 8;
    const long r0 = i0 + 2 * wave;
    const double *p0 = Winv + r0 * n + 2 * lane, *p1 = p0 + n;
    const int nq = (int)(n / 128);
    const double2_t zero2 = {0.0, 0.0};
    double2_t x0p[SR_PF], x1p[SR_PF];
    if (mode != 2) {
#pragma unroll
        for (int q = 0; q < SR_PF; ++q) {
            x0p[q] = q < nq ? *(const double2_t *)(p0 + 128 * q) : zero2;
            x1p[q] = q < nq ? *(const double2_t *)(p1 + 128 * q) : zero2;
        }
    }
    if (mode != 2) {
        // k_m[j]: the arithmetic of the cross-covariance kernels (inputs divided first, squares summed in dimension order)
        for (long j = tid; j < n; j += 256) {
            double acc[MV];
#pragma unroll
            for (int m = 0; m < MV; ++m) acc[m] = 0.0;
            const bool live = j < Mz;
            if (live) {
                for (int d = 0; d < D; ++d) {
                    const double b = Zs[j * D + d];
#pragma unroll
                    for (int m = 0; m < MV; ++m) {
                        if (m < M) {
                            const double df = xs_s[m * D + d] - b;
                            acc[m] = fma(df, df, acc[m]);
                        }
                    }
                }
            }
#pragma unroll
            for (int m = 0; m < MV; ++m) ks[m * SR_MAXZ + j] = (live && m < M) ? gp_k_of_r2(kp.kernel, kp.variance, acc[m]) : 0.0;
        }
        __syncthreads();
        // b_m[i] = sum_j Winv[i, j] k_m[j] on this wave's two rows, the column pairs added in q order (columns past n: zeros)
        double a0[MV], a1[MV], c0[MV], c1[MV];
#pragma unroll
        for (int m = 0; m < MV; ++m) a0[m] = a1[m] = c0[m] = c1[m] = 0.0;
#pragma unroll
        for (int q = 0; q < SR_PF; ++q) {
            if (q < nq) {
#pragma unroll
                for (int m = 0; m < MV; ++m) {
                    const double2_t k = *(const double2_t *)&ks[m * SR_MAXZ + 2 * lane + 128 * q];
                    a0[m] = fma(x0p[q][0], k[0], a0[m]);
                    a1[m] = fma(x0p[q][1], k[1], a1[m]);
                    c0[m] = fma(x1p[q][0], k[0], c0[m]);
                    c1[m] = fma(x1p[q][1], k[1], c1[m]);
                }
            }
        }
#pragma unroll 4
        for (int q = SR_PF; q < nq; ++q) {
            const double2_t x0 = *(const double2_t *)(p0 + 128 * q), x1 = *(const double2_t *)(p1 + 128 * q);
#pragma unroll
            for (int m = 0; m < MV; ++m) {
                const double2_t k = *(const double2_t *)&ks[m * SR_MAXZ + 2 * lane + 128 * q];
                a0[m] = fma(x0[0], k[0], a0[m]);
                a1[m] = fma(x0[1], k[1], a1[m]);
                c0[m] = fma(x1[0], k[0], c0[m]);
                c1[m] = fma(x1[1], k[1], c1[m]);
            }
        }
#pragma unroll
        for (int m = 0; m < MV; ++m) {
            const double sa = sr_wave_sum(a0[m] + a1[m]), sb = sr_wave_sum(c0[m] + c1[m]);
            if (lane == 0) {
                bs[m][2 * wave] = sa;
                bs[m][2 * wave + 1] = sb;
            }
        }
    }
    __syncthreads();
    // row i of location m: its terms of k . b and k . w, and the weights g w_i, -2 g b_i of the two gradients_X sums
    // (stationary.py:336-364; g = dK_dr / r, 0 where the distance is exactly 0: _inv_dist :251-258)
    if (tid < MV * RB) {
        const int m = tid / RB, r = tid % RB;
        const long i = i0 + r;
        double gwv = 0.0, gbv = 0.0, kbv = 0.0, kwv = 0.0;
        if (m < M && i < Mz) {
            double s = 0.0;
            for (int d = 0; d < D; ++d) {
                const double df = xs_s[m * D + d] - Zs[i * D + d];
                s = fma(df, df, s);
            }
            double kv, gv;
            gp_k_and_g(kp.kernel, kp.variance, s, kv, gv);
            if (s == 0.0) gv = 0.0;
            const double wi = w[i];
            gwv = gv * wi;
            if (mode != 2) {
                const double b = bs[m][r], k = ks[m * SR_MAXZ + i];
                gbv = gv * (-2.0 * b);
                kbv = k * b;
                kwv = k * wi;
            }
        }
        gw[m][r] = gwv;
        gb[m][r] = gbv;
        kb[m][r] = kbv;
        kw[m][r] = kwv;
    }
    __syncthreads();
    double *const grow = gpart + (long)blockIdx.x * SR_GROW;
    if (mode != 0)
        for (int t = tid; t < M * D; t += 256) {
            const int m = t / D, d = t % D;
            double sm = 0.0, sv = 0.0;
            for (int r = 0; r < RB; ++r) {
                const long i = i0 + r;
                if (i < Mz) {
                    const double dq = xs_s[t] - Zs[i * D + d];
                    sm = fma(gw[m][r], dq, sm);
                    sv = fma(gb[m][r], dq, sv);
                }
            }
            grow[t] = sm;
            grow[SR_XS + t] = sv;
        }
    if (mode != 2 && tid < M) {
        double s1 = 0.0, s2 = 0.0;
        for (int r = 0; r < RB; ++r) {
            s1 += kb[tid][r];
            s2 += kw[tid][r];
        }
        grow[2 * SR_XS + tid] = s1;
        grow[2 * SR_XS + ROWS_WIDE_M + tid] = s2;
    }
    // the arrival counter of rows_finish_kernel (onerow.hip): device-scope atomic, counted from this pass's base, never reset
    __threadfence();
    __syncthreads();
    if (tid == 0) last_s = (atomicAdd(counter, 1u) - counter_base == gridDim.x - 1) ? 1 : 0;   // (unsigned: wraps with the base)
    __syncthreads();
    if (!last_s) return;
    __threadfence();
    // the workgroups' sums in eight interleaved slices: slice j adds the workgroups j, j + 8, ... in order, then the slices are
    // added in order.  Values: [M D of d mean | M D of d var] (modes 1, 2), then [M of k . b | M of k . w] (modes 0, 1)
    const int ng = mode != 0 ? 2 * M * D : 0;
    const int ntot = ng + (mode != 2 ? 2 * M : 0);
    for (int idx = tid; idx < 8 * ntot; idx += 256) {
        const int v = idx % ntot, j = idx / ntot;
        int off;
        if (v < ng)
            off = v < M * D ? v : SR_XS + (v - M * D);
        else
            off = (v - ng) < M ? 2 * SR_XS + (v - ng) : 2 * SR_XS + ROWS_WIDE_M + (v - ng - M);
        fin_s[j][v] = sr_strided_sum(gpart + off, SR_GROW, j, 8, (int)gridDim.x);
    }
    __syncthreads();
    for (int v = tid; v < ntot; v += 256) {
        double s = 0.0;
        for (int j = 0; j < 8; ++j) s += fin_s[j][v];
        res_s[v] = v < ng ? s / kp.ls[v % D] : s;   // (x - z) / l^2 = scaled difference / l
    }
    __syncthreads();
    constexpr int ML = ROWS_WIDE_M;
    if (tid < M) {
        const int m = tid;
        // (the host-visible block is written once and never read here: everything the chain rule needs stays in LDS)
        double *dm = out + 3 * ML + m * D, *dv = out + 3 * ML + ML * D + m * D, *da = out + 3 * ML + 2 * ML * D + m * D;
        const double *gm = res_s + m * D, *gv = res_s + M * D + m * D;
        double *ga = da_s + m * D;
        if (mode != 0)
            for (int d = 0; d < D; ++d) {
                dm[d] = gm[d];
                if (mode == 1) dv[d] = gv[d];
            }
        if (mode != 2) {
            const double mean = res_s[ng + M + m];
            const double var = fmax(kss - res_s[ng + m], 1e-15) + noise_add;   // posterior.py:248 clips before the noise is added
            out[m] = mean;
            out[ML + m] = var;
            if (aq.on) {
                double f, c_m, c_s, ds_scale;
                acq_terms(aq.type, aq.par, aq.fmin, aq.y_mean, aq.y_std, mean, var, f, c_m, c_s, ds_scale);
                double neg = -f;
                if (mode == 1)
                    for (int d = 0; d < D; ++d) ga[d] = -(c_m * (gm[d] * aq.y_std) + c_s * (gv[d] * ds_scale));
                if (aq.lp) {
                    const double *x = xraw_s + m * D;
                    neg = mode == 1 ? lp_value_grad(neg, ga, x, D, aq.Xb, aq.nb, aq.r0, aq.s0, aq.transform)
                                    : lp_value(neg, x, D, aq.Xb, aq.nb, aq.r0, aq.s0, aq.transform);
                }
                out[2 * ML + m] = neg;
                if (mode == 1)
                    for (int d = 0; d < D; ++d) da[d] = ga[d];
            }
        }
    }
    __syncthreads();
    if (tid == 0) out[ROWS_OUT_DOUBLES] = ticket;   // this pass is complete (the host checks the ticket behind the results)
}

// Zs[j, d] = Z[j, d] / l_d, j < Mz
__global__ void sparse_scale_z_kernel(const double *Z, long Mz, KernParams kp, double *Zs) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < Mz * kp.D) Zs[e] = Z[e] / kp.ls[e % kp.D];
}
void launch_sparse_scale_z(hipStream_t s, const double *Z, long Mz, const KernParams &kp, double *Zs) {
    GP_LAUNCH(sparse_scale_z_kernel, dim3((unsigned)((Mz * kp.D + 255) / 256)), dim3(256), 0, s, Z, Mz, kp, Zs);
}

void launch_sparse_rows(hipStream_t s, const double *Winv, long n, long Mz, const RowsX &rx, const KernParams &kp, const double *Zs,
                        const double *w, int mode, double kss, double noise_add, const RowsAcq &aq, double *gpart,
                        const PassReport &r) {
    const unsigned grid = sparse_rows_grid(Mz);
#define SR_GO(MV)                                                                                                                     \
    GP_LAUNCH(sparse_rows_kernel<MV>, dim3(grid), dim3(256), 0, s, Winv, n, Mz, rx, kp, Zs, w, mode, kss, noise_add, aq, gpart, r.counter, \
              r.base, r.out, r.ticket)
    if (rx.M == 1) SR_GO(1);
    else if (rx.M <= ROWS_MAX_M) SR_GO(ROWS_MAX_M);
    else SR_GO(ROWS_WIDE_M);
#undef SR_GO
}
