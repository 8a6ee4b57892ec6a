// The sparse model's posterior covariance between a block of locations and a RESIDENT second point set, as ONE launch over
// G = K(X2, Z) woodbury_inv.
//
// Entropy search asks, per candidate x, for the covariance between x and its R representers X2 (posterior.py:229-232 over
// _predictive_variable = Z, off-diagonal block):
//     cov[i, r] = k(x1_i, x2_r) - sum_j G[r, j] k(x1_i, z_j)
// G depends on the fit and on X2 only and is cached by the caller (api_sparse_cov.hip); what is left per call is matrix-vector work
// bound by one read of the R x Mz matrix (0.8 MB at R = 50 and the Mz = 2048 cap).
//
//   sparse_cov_between_kernel   a workgroup takes SPARSE_COV_RB rows of G (blockIdx.x) and a block of up to eight locations
//                               (blockIdx.y).  The rows' first columns are requested at once; it generates k(x, Z) of its
//                               locations into LDS from the pre-scaled Zs (16 KB per location at the cap, as sparse_rows_kernel),
//                               forms G k on its rows -- two rows per wave, all locations of the block from one read of the rows
//                               --, and one thread per (location, row) subtracts the sum from k(x, x2_r) and writes it.
//
// Every output (i, r) has ONE writer and a fixed summation order: a lane adds the column pairs 2 lane + 128 q in q order (even and
// odd columns apart), the two are added, the wave's 64 lanes by the shuffle tree.  Nothing of it depends on the number of
// locations, on a location's slot, on the block it rides in or on how R is cut into workgroups: the same bits whatever the company.
// Up to ROWS_WIDE_M locations travel in the kernel arguments and the results land in host-visible memory, the last workgroup to
// arrive writing the pass's ticket behind them: no copy commands on either side of the launch.  More locations are read from the
// device and written to it, block by block, by the same body.
#include "gphip_internal.h"

#define SC_MAXZ 2048      // GP_SPARSE_MAX_INDUCING (include/gphip.h): columns of k kept in LDS per location
#define SC_RB SPARSE_COV_RB

__device__ __forceinline__ double sc_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}

// grid = (sparse_cov_grid(R), location blocks) workgroups of 256 threads.  G is Rpad x n row-major (n = Mz rounded up to the tile,
// at most SC_MAXZ; Rpad = R rounded up to the tile, zero rows in the padding), Zs [Mz, D] and X2s [R, D] the inducing inputs and
// the second point set already divided by the lengthscales.  X1 null: the rx.M locations of rx (gridDim.y = 1), out [rx.M, ldo]
// host-visible, and the last workgroup to arrive writes `ticket` to *tick.  Otherwise block y takes the rows [MV y, MV y + MV) of
// X1 [M1, D] on the device and writes those rows of out [M1, ldo]; no counter.
template <int MV>
__global__ __launch_bounds__(256) void sparse_cov_between_kernel(const double *G, long n, long Mz, long R, const double *X2s, RowsX rx,
                                                                 const double *X1, long M1, KernParams kp, const double *Zs,
                                                                 double *out, long ldo, unsigned int *counter,
                                                                 unsigned int counter_base, double *tick, double ticket) {
    __shared__ __attribute__((aligned(16))) double ks[MV * SC_MAXZ];
    __shared__ double xs_s[MV * GP_MAX_D];
    __shared__ double bs[MV][SC_RB];
    __shared__ int last_s;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int D = kp.D;
    const long m0 = (long)blockIdx.y * MV;
    const int M = X1 ? (int)(M1 - m0 < MV ? M1 - m0 : MV) : rx.M;
    const long i0 = (long)blockIdx.x * SC_RB;
    for (int i = tid; i < M * D; i += 256) xs_s[i] = (X1 ? X1[m0 * D + i] : rx.xs[i]) / kp.ls[i % D];
    __syncthreads();
    // this wave's two rows of G, r0 and r0 + 1 (r0 + 1 < Rpad: the grid covers ceil(R / SC_RB) SC_RB <= Rpad rows); a lane holds
    // the column pairs 2 lane + 128 q.  The first SC_PF of them are requested here, before k exists.
    constexpr int SC_PF = MV > ROWS_MAX_M ? 4 : 8;
    const long r0 = i0 + 2 * wave;
    const double *p0 = G + r0 * n + 2 * lane, *p1 = p0 + n;
    const int nq = (int)(n / 128);
    const double2_t zero2 = {0.0, 0.0};
    double2_t x0p[SC_PF], x1p[SC_PF];
#pragma unroll
    for (int q = 0; q < SC_PF; ++q) {
        x0p[q] = q < nq ? *(const double2_t *)(p0 + 128 * q) : zero2;
        x1p[q] = q < nq ? *(const double2_t *)(p1 + 128 * q) : zero2;
    }
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
        for (int m = 0; m < MV; ++m) ks[m * SC_MAXZ + j] = (live && m < M) ? gp_k_of_r2(kp.kernel, kp.variance, acc[m]) : 0.0;
    }
    __syncthreads();
    // (G k_m)[r] on this wave's two rows, the column pairs added in q order (columns past Mz: zeros of k)
    double a0[MV], a1[MV], c0[MV], c1[MV];
#pragma unroll
    for (int m = 0; m < MV; ++m) a0[m] = a1[m] = c0[m] = c1[m] = 0.0;
#pragma unroll
    for (int q = 0; q < SC_PF; ++q) {
        if (q < nq) {
#pragma unroll
            for (int m = 0; m < MV; ++m) {
                const double2_t k = *(const double2_t *)&ks[m * SC_MAXZ + 2 * lane + 128 * q];
                a0[m] = fma(x0p[q][0], k[0], a0[m]);
                a1[m] = fma(x0p[q][1], k[1], a1[m]);
                c0[m] = fma(x1p[q][0], k[0], c0[m]);
                c1[m] = fma(x1p[q][1], k[1], c1[m]);
            }
        }
    }
#pragma unroll 4
    for (int q = SC_PF; q < nq; ++q) {
        const double2_t x0 = *(const double2_t *)(p0 + 128 * q), x1 = *(const double2_t *)(p1 + 128 * q);
#pragma unroll
        for (int m = 0; m < MV; ++m) {
            const double2_t k = *(const double2_t *)&ks[m * SC_MAXZ + 2 * lane + 128 * q];
            a0[m] = fma(x0[0], k[0], a0[m]);
            a1[m] = fma(x0[1], k[1], a1[m]);
            c0[m] = fma(x1[0], k[0], c0[m]);
            c1[m] = fma(x1[1], k[1], c1[m]);
        }
    }
#pragma unroll
    for (int m = 0; m < MV; ++m) {
        const double sa = sc_wave_sum(a0[m] + a1[m]), sb = sc_wave_sum(c0[m] + c1[m]);
        if (lane == 0) {
            bs[m][2 * wave] = sa;
            bs[m][2 * wave + 1] = sb;
        }
    }
    __syncthreads();
    // one thread per (location, row): k(x1_m, x2_r) in the cross-covariance kernels' arithmetic, minus the row's sum
    if (tid < MV * SC_RB) {
        const int m = tid / SC_RB, r = tid % SC_RB;
        const long i = i0 + r;
        if (m < M && i < R) {
            double s = 0.0;
            for (int d = 0; d < D; ++d) {
                const double df = xs_s[m * D + d] - X2s[i * D + d];
                s = fma(df, df, s);
            }
            out[(m0 + m) * ldo + i] = gp_k_of_r2(kp.kernel, kp.variance, s) - bs[m][r];
        }
    }
    if (!counter) return;
    // the arrival counter of the fused rows passes (onerow.hip): device-scope atomic, counted from this pass's base, never reset
    __threadfence();
    __syncthreads();
    if (tid == 0) last_s = (atomicAdd(counter, 1u) - counter_base == gridDim.x - 1) ? 1 : 0;   // (unsigned: wraps with the base)
    __syncthreads();
    if (last_s && tid == 0) {
        __threadfence();
        *tick = ticket;   // this pass is complete (the host checks the ticket after the sync)
    }
}

void launch_sparse_cov_rows(hipStream_t s, const double *G, long n, long Mz, long R, const double *X2s, const RowsX &rx,
                            const KernParams &kp, const double *Zs, double *out, const PassReport &r) {
    const dim3 grid(sparse_cov_grid(R));
#define SC_GO(MV)                                                                                                                    \
    GP_LAUNCH(sparse_cov_between_kernel<MV>, grid, dim3(256), 0, s, G, n, Mz, R, X2s, rx, (const double *)nullptr, 0L, kp, Zs, out, R, \
              r.counter, r.base, r.out + ROWS_OUT_DOUBLES, r.ticket)
    if (rx.M == 1) SC_GO(1);
    else if (rx.M <= ROWS_MAX_M) SC_GO(ROWS_MAX_M);
    else SC_GO(ROWS_WIDE_M);
#undef SC_GO
}

void launch_sparse_cov_table(hipStream_t s, const double *G, long n, long Mz, long R, const double *X2s, const double *X1, long M1,
                             const KernParams &kp, const double *Zs, double *out) {
    RowsX none{};   // (the locations come from X1)
    const long per = 32768L * ROWS_WIDE_M;   // locations per launch: gridDim.y stays below 65536
    for (long m0 = 0; m0 < M1; m0 += per) {
        const long mc = M1 - m0 < per ? M1 - m0 : per;
        const dim3 grid(sparse_cov_grid(R), (unsigned)((mc + ROWS_WIDE_M - 1) / ROWS_WIDE_M));
        GP_LAUNCH(sparse_cov_between_kernel<ROWS_WIDE_M>, grid, dim3(256), 0, s, G, n, Mz, R, X2s, none, X1 + m0 * kp.D, mc, kp, Zs,
                  out + m0 * R, R, (unsigned int *)nullptr, 0u, (double *)nullptr, 0.0);
    }
}
