// The acquisition optimiser's one-row calls as THREE launches over the explicit inverse factor.
//
// scipy's L-BFGS-B evaluates acquisition_function_withGradients one location at a time, hundreds of times between two fits
// (GPyOpt/GPyOpt/optimization/optimizer.py:36-61 -> acquisitions/base.py:42-50 -> models/gpmodel.py:131-142 ->
// GPy/GPy/core/gp.py:407-454 + posterior.py:273-302).  Per location x the reference needs
//     k* = K(X, x),  mean = k*^T alpha,  w = L^-1 k* (dtrtrs),  var = kss - |w|^2,  beta = Ky^-1 k*,
//     d mean / dx = gradients_X(alpha^T, x, X),  d var / dx = gradients_X(-2 beta^T, x, X)       (stationary.py:336-364)
// and the EI / LCB / MPI (+ local penalisation) chain rule on top.  With the inverse factor Li = L^-1 kept from the potri-
// equivalent (api_solve.hip, ensure_linv; lower triangular, row-major) this is matrix-vector work bound by reading the lower
// triangle of Li twice (2 x 8 N^2 / 2 bytes: 2.15 GB at N = 16384):
//
//   rows_forward_kernel    w = Li k*           row dots; k* generated on the fly per 1024-column chunk (never stored)
//   rows_backward_kernel   beta = Li^T w       column sums over the same tiles; |w|^2 per row block on the way
//   rows_finish_kernel     beta -> the two gradients_X sums over the training points, then -- in the last workgroup to arrive --
//                          mean, variance, acquisition, penaliser, written straight into the caller's pinned result block
//
// Up to ROWS_MAX_M locations share a pass (MV = 1 or 4), 5 .. ROWS_WIDE_M a WIDE pass (MV = 8: rows_forward_wide_kernel and the
// MV = 8 instances of the other kernels); per location the arithmetic and its order are the same in all of them.
// x travels in the kernel arguments and the results land in host-visible memory: no copy commands either side of the launches.
// The smallm.hip route walked ~22 panels x 2 dependent launches for the same substitution (1.36 ms per gradient call at
// N = 16384, 0.18 ms at N = 512).  A posterior-only call (no gradient) is forward + finish: two launches, one read of Li.
//
// Tiling: row blocks of 128 rows x chunks of 1024 columns of the lower triangle (row block R has R / 8 + 1 chunks, the last
// one cut at the diagonal tile's end).  Every partial sum has ONE writer and is reduced in a fixed order: bitwise repeatable.
#include "rows_body.h"

long rows_tiles(int nt) {
    long t = 0;
    for (int R = 0; R < nt; ++R) t += rw_nch(R);
    return t;
}

// ---- the single model's kernels over the shared bodies (rows_body.h) --------------------------------------------------------------------
template <int MV, int RB, bool NT>
__global__ __launch_bounds__(256) void rows_forward_kernel(const double *Li, long ld, RowsX rx, KernParams kp, const double *X, long N,
                                                           const double *alpha, double *wpart, long Npad, int nt,
                                                           double *meanpart) {
    rows_forward_body<MV, RB, NT>(blockIdx.x, Li, ld, rx, kp, X, N, alpha, wpart, Npad, nt, meanpart);
}
template <int MV, int RB, bool NT>
__global__ __launch_bounds__(256) void rows_backward_kernel(const double *Li, long ld, const double *wpart, long Npad, int M,
                                                            double *bpart, double *vpart) {
    rows_backward_body<MV, RB, NT>(blockIdx.x, Li, ld, wpart, Npad, M, bpart, vpart);
}
template <int MV, bool MEAN, bool MES>
__global__ __launch_bounds__(256) void rows_finish_kernel(RowsX rx, KernParams kp, const double *X, long N, const double *alpha,
                                                          const double *wpart, const double *bpart, const double *meanpart,
                                                          const double *vpart, long Npad, int nt, int rbh, int want_grad,
                                                          double kss, double noise_add, RowsAcq aq, double *gpart,
                                                          unsigned int *counter, unsigned int counter_base, double *out,
                                                          double ticket, const double *mA, const double *mb) {
    if (!rows_finish_body<MV, MEAN, MES>(blockIdx.x, gridDim.x, rx, kp, X, N, alpha, wpart, bpart, meanpart, vpart, Npad, nt, rbh, want_grad,
                                    kss, noise_add, aq, gpart, counter, counter_base, out, mA, mb))
        return;
    if (threadIdx.x == 0) out[ROWS_OUT_DOUBLES] = ticket;   // this pass is complete (the host checks the ticket behind the results)
}


// ---- forward, wide: the same sums for up to ROWS_WIDE_M locations in ONE read of Li -------------------------------------------------------
// One level of the rw_wave_sum tree for two values at once: lanes with bit o clear keep p[i] + p[i + o], lanes with it set keep
// q[i] + q[i - o] -- what the tree's lane i - o computes for q, operands swapped, and floating-point addition is commutative.
__device__ __forceinline__ double rw_fold(double p, double q, int lane, int o) {
    const bool up = lane & o;
    return (up ? q : p) + __shfl_xor(up ? p : q, o);
}
// The 16 sums of a row pair (v[2 m + row]) through ONE tree: 8 + 4 + 2 + 1 folds, then the last two levels on the survivor.  Lane 4 g
// ends up with rw_wave_sum's lane-0 value of v[rw_fold_index(4 g)], bit for bit (17 shuffles for 16 x 6).
__device__ __forceinline__ double rw_wave_sum16(const double (&v)[16], int lane) {
    double a[8], b[4];
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = rw_fold(v[2 * k], v[2 * k + 1], lane, 32);
#pragma unroll
    for (int k = 0; k < 4; ++k) b[k] = rw_fold(a[2 * k], a[2 * k + 1], lane, 16);
    const double c0 = rw_fold(b[0], b[1], lane, 8), c1 = rw_fold(b[2], b[3], lane, 8);
    double s = rw_fold(c0, c1, lane, 4);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 1);
    return s;
}
__device__ __forceinline__ int rw_fold_index(int lane) {   // lane bits 5, 4, 3, 2 -> index bits 0, 1, 2, 3
    return ((lane >> 5) & 1) | (((lane >> 4) & 1) << 1) | (((lane >> 3) & 1) << 2) | (((lane >> 2) & 1) << 3);
}

// rows_forward_kernel for MV = ROWS_WIDE_M.  k* stays in LDS (64 KiB: two workgroups per CU) and is re-read per row pair -- eight
// locations' worth in registers would be 256 VGPRs -- and the 16 wave sums of a row pair share one tree.  Per location the
// arithmetic is rows_forward_kernel's, in its order: the same bits, whatever the slot and the company.
template <int RB, bool NT>
__global__ __launch_bounds__(256) void rows_forward_wide_kernel(const double *Li, long ld, RowsX rx, KernParams kp, const double *X,
                                                                long N, const double *alpha, double *wpart, long Npad, int nt,
                                                                double *meanpart) {
    constexpr int MV = ROWS_WIDE_M;
    __shared__ __attribute__((aligned(16))) double ks[MV][RW_CW];
    __shared__ double xs_s[ROWS_MAX_XS];
    __shared__ double red[4];
    constexpr int SUB = GP_TILE / RB;
    int R, C;
    rw_decode((int)blockIdx.x / SUB, R, C);
    const int sub = (int)blockIdx.x % SUB;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int D = kp.D, M = rx.M;
    const long c0 = (long)C * RW_CW;
    const int klim = min(RW_CW, (R + 1) * GP_TILE - (int)c0);   // a multiple of 128
    for (int i = tid; i < M * D; i += 256) xs_s[i] = rx.xs[i] / kp_div(kp, i % D);
    __syncthreads();
    for (int j = tid; j < RW_CW; j += 256) {
        const long i = c0 + j;
        double acc[MV];
#pragma unroll
        for (int m = 0; m < MV; ++m) acc[m] = kp.gower ? 1.0 : 0.0;
        const bool live = j < klim && i < N;
        if (live) {
            for (int d = 0; d < D; ++d) {
                const double b = X[i * D + d] / kp_div(kp, d);
#pragma unroll
                for (int m = 0; m < MV; ++m) {
                    if (m < M) {
                        const double df = xs_s[m * D + d] - b;
                        if (kp.gower) {
                            const double r = kp.gdisc[d] ? (df != 0.0 ? 1.0 : 0.0) : fabs(df);
                            acc[m] *= gp_k_of_r2(kp.kernel, kp.variance, r * r);
                        } else {
                            acc[m] = fma(df, df, acc[m]);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int m = 0; m < MV; ++m)
            ks[m][j] = (live && m < M) ? (kp.gower ? acc[m] : gp_k_of_r2(kp.kernel, kp.variance, acc[m])) : 0.0;
    }
    __syncthreads();
    if (R == nt - 1 && sub == 0) {   // the last row block meets every chunk: it carries the mean's partial sums
        for (int m = 0; m < M; ++m) {
            double s = 0.0;
            for (int j = tid; j < klim; j += 256)
                if (c0 + j < N) s = fma(ks[m][j], alpha[c0 + j], s);
            s = rw_block_sum(s, red);
            if (tid == 0) meanpart[C * MV + m] = s;
        }
    }
    const long rbase = (long)R * GP_TILE + sub * RB + wave * (RB / 4);
    const double2_t zero2 = {0.0, 0.0};
    const int slot = rw_fold_index(lane);
    const bool writer = (lane & 3) == 0 && (slot >> 1) < M;
    double *const o = wpart + ((long)C * MV + (slot >> 1)) * Npad + rbase + (slot & 1);
    // The next row pair's loads go out before this one's products, and the products are held to one location at a time
    // (sched_barrier): left alone the compiler gathers all eight locations' k* reads, 364 registers and one workgroup per CU
    // (profiles/rows_wide_resources.txt).
    const double *const pl = Li + rbase * ld + c0 + 2 * lane;
    double2_t x0[RW_Q], x1[RW_Q], n0[RW_Q], n1[RW_Q];
#pragma unroll
    for (int q = 0; q < RW_Q; ++q) {
        x0[q] = (128 * q < klim) ? rw_load2<NT>(pl + 128 * q) : zero2;
        x1[q] = (128 * q < klim) ? rw_load2<NT>(pl + ld + 128 * q) : zero2;
    }
    for (int r = 0; r < RB / 4; r += 2) {
        if (r + 2 < RB / 4) {
            const double *p0 = pl + (long)(r + 2) * ld;
#pragma unroll
            for (int q = 0; q < RW_Q; ++q) {
                n0[q] = (128 * q < klim) ? rw_load2<NT>(p0 + 128 * q) : zero2;
                n1[q] = (128 * q < klim) ? rw_load2<NT>(p0 + ld + 128 * q) : zero2;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        double v[2 * MV];
#pragma unroll
        for (int m = 0; m < MV; ++m) {
            double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;
#pragma unroll
            for (int q = 0; q < RW_Q; ++q) {
                const double2_t k = *(const double2_t *)&ks[m][2 * lane + 128 * q];
                a0 = fma(x0[q][0], k[0], a0);
                a1 = fma(x0[q][1], k[1], a1);
                b0 = fma(x1[q][0], k[0], b0);
                b1 = fma(x1[q][1], k[1], b1);
            }
            v[2 * m] = a0 + a1;
            v[2 * m + 1] = b0 + b1;
            __builtin_amdgcn_sched_barrier(0);
        }
        const double s = rw_wave_sum16(v, lane);
        if (writer) o[r] = s;
        if (r + 2 < RB / 4) {
#pragma unroll
            for (int q = 0; q < RW_Q; ++q) {
                x0[q] = n0[q];
                x1[q] = n1[q];
            }
        }
    }
}


// ---- the mean's gradient alone ---------------------------------------------------------------------------------------------------------
// d mean / dx = gradients_X(alpha^T, x, X) (gp.py:433-438 over stationary.py:336-364) needs neither L^-1 nor k* products: one pass
// over the training points.  What estimate_L's L-BFGS-B asks for, one location at a time and D + 1 times per step (it differentiates by
// forward differences, batch_local_penalization.py:55-67).  grid = ceil(N / 256); the last workgroup to arrive adds the workgroups'
// sums in workgroup order and writes dmdx [M, D] at out + 3 MV (the place rows_finish_kernel writes it).
// MEAN: the instances of a model with a mean function add its A [D] (rows_finish_body)
template <int MV, bool MEAN>
__global__ __launch_bounds__(256) void rows_mean_grad_kernel(RowsX rx, KernParams kp, const double *X, long N, const double *alpha,
                                                             double *gpart, unsigned int *counter, unsigned int counter_base,
                                                             double *out, double ticket, const double *mA) {
    __shared__ double xs_s[ROWS_MAX_XS];
    __shared__ double sh[4][ROWS_MAX_XS];
    __shared__ double fin_s[8][ROWS_MAX_XS];
    __shared__ int last_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int D = kp.D, M = rx.M, nval = M * D;
    for (int i = tid; i < nval; i += 256) xs_s[i] = rx.xs[i] / kp.ls[i % D];
    __syncthreads();
    const long n = (long)blockIdx.x * 256 + tid;
    const bool live = n < N;
    const double a = live ? alpha[n] : 0.0;
    for (int m = 0; m < M; ++m) {
        double s = 0.0;
        if (live)
            for (int d = 0; d < D; ++d) {
                const double df = xs_s[m * D + d] - X[n * D + d] / kp.ls[d];
                s = fma(df, df, s);
            }
        double kv, gv;
        gp_k_and_g(kp.kernel, kp.variance, s, kv, gv);
        if (s == 0.0) gv = 0.0;   // invdist = 0 where the distance is exactly 0 (stationary.py:251-258)
        const double tm = live ? gv * a : 0.0;
        for (int d = 0; d < D; ++d) {
            const double dq = live ? xs_s[m * D + d] - X[n * D + d] / kp.ls[d] : 0.0;
            const double v = rw_wave_sum(tm * dq);
            if (lane == 0) sh[wave][m * D + d] = v;
        }
    }
    __syncthreads();
    if (tid < nval) gpart[(long)blockIdx.x * RW_GROW + tid] = ((sh[0][tid] + sh[1][tid]) + sh[2][tid]) + sh[3][tid];
    __threadfence();
    __syncthreads();
    if (tid == 0) last_s = (atomicAdd(counter, 1u) - counter_base == gridDim.x - 1) ? 1 : 0;   // (unsigned: wraps with the base)
    __syncthreads();
    if (!last_s) return;
    __threadfence();
    for (int idx = tid; idx < 8 * nval; idx += 256) {
        const int v = idx % nval, j = idx / nval;
        fin_s[j][v] = rw_strided_sum(gpart + v, RW_GROW, j, 8, (int)gridDim.x);
    }
    __syncthreads();
    for (int v = tid; v < nval; v += 256) {
        double s = 0.0;
        for (int j = 0; j < 8; ++j) s += fin_s[j][v];
        const double gm = s / kp.ls[v % D];   // (x - x') / l^2 = scaled difference / l
        out[3 * MV + v] = MEAN ? gm + mA[v % D] : gm;
    }
    __syncthreads();
    if (tid == 0) out[ROWS_OUT_DOUBLES] = ticket;
}

void launch_rows_mean_grad(hipStream_t s, const RowsX &rx, const KernParams &kp, const double *X, long N, const double *alpha,
                           const RowsWork &w, const PassReport &r, const RowsMean &mf) {
    const unsigned grid = rows_mean_grad_grid(N);
#define RW_MG(MV, MEAN) GP_LAUNCH((rows_mean_grad_kernel<MV, MEAN>), dim3(grid), dim3(256), 0, s, rx, kp, X, N, alpha, w.gpart, r.counter, r.base, r.out, r.ticket, mf.A)
    if (rx.M == 1) {
        if (mf.on) RW_MG(1, true); else RW_MG(1, false);
    } else if (rx.M > ROWS_MAX_M) {
        if (mf.on) RW_MG(ROWS_WIDE_M, true); else RW_MG(ROWS_WIDE_M, false);
    } else {
        if (mf.on) RW_MG(ROWS_MAX_M, true); else RW_MG(ROWS_MAX_M, false);
    }
#undef RW_MG
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------------
size_t rows_gpart_elems(long N) { return (size_t)std::max(rows_finish_grid(N), rows_mean_grad_grid(N)) * RW_GROW; }

int rows_block_height(int nt) { return nt <= 16 ? 32 : GP_TILE; }

template <int MV, int RB, bool NT>
static void launch_rows_t(hipStream_t s, const double *Li, long Npad, const RowsX &rx, const KernParams &kp, const double *X, long N,
                          const double *alpha, int want_grad, double kss, double noise_add, const RowsAcq &aq, const RowsWork &w,
                          const PassReport &r, bool forward_only, const RowsMean &mf) {
    const int nt = (int)(Npad / GP_TILE);
    const unsigned tiles = (unsigned)rows_tiles(nt) * (GP_TILE / RB);
    const unsigned fin = rows_finish_grid(N);
    if constexpr (MV > ROWS_MAX_M)
        GP_LAUNCH((rows_forward_wide_kernel<RB, NT>), dim3(tiles), dim3(256), 0, s, Li, Npad, rx, kp, X, N, alpha, w.wpart, Npad, nt, w.meanpart);
    else
        GP_LAUNCH((rows_forward_kernel<MV, RB, NT>), dim3(tiles), dim3(256), 0, s, Li, Npad, rx, kp, X, N, alpha, w.wpart, Npad, nt, w.meanpart);
    if (forward_only) return;
    if (want_grad)
        GP_LAUNCH((rows_backward_kernel<MV, RB, NT>), dim3(tiles), dim3(256), 0, s, Li, Npad, w.wpart, Npad, rx.M, w.bpart, w.vpart);
#define RW_FIN(MEAN, MES, A, B)                                                                                                      \
    GP_LAUNCH((rows_finish_kernel<MV, MEAN, MES>), dim3(fin), dim3(256), 0, s, rx, kp, X, N, alpha, w.wpart, w.bpart, w.meanpart, w.vpart, \
              Npad, nt, RB, want_grad, kss, noise_add, aq, w.gpart, r.counter, r.base, r.out, r.ticket, (const double *)(A), (const double *)(B))
    const bool mes = aq.on && aq.type == GP_ACQ_MES;   // the rule's own instances (rows_body.h)
    if (mf.on) {
        if (mes) RW_FIN(true, true, mf.A, mf.b); else RW_FIN(true, false, mf.A, mf.b);
    } else {
        if (mes) RW_FIN(false, true, nullptr, nullptr); else RW_FIN(false, false, nullptr, nullptr);
    }
#undef RW_FIN
}

static void launch_rows_any(hipStream_t s, const double *Li, long Npad, const RowsX &rx, const KernParams &kp, const double *X, long N,
                            const double *alpha, int want_grad, double kss, double noise_add, const RowsAcq &aq, const RowsWork &w,
                            const PassReport &r, int nt_loads, bool forward_only, const RowsMean &mf) {
    const bool low = rows_block_height((int)(Npad / GP_TILE)) == 32;
#define RW_GO(MV, RB, NT) launch_rows_t<MV, RB, NT>(s, Li, Npad, rx, kp, X, N, alpha, want_grad, kss, noise_add, aq, w, r, forward_only, mf)
    if (rx.M == 1) {
        if (low) RW_GO(1, 32, false);
        else if (nt_loads) RW_GO(1, GP_TILE, true);
        else RW_GO(1, GP_TILE, false);
    } else if (rx.M <= ROWS_MAX_M) {
        if (low) RW_GO(ROWS_MAX_M, 32, false);
        else if (nt_loads) RW_GO(ROWS_MAX_M, GP_TILE, true);
        else RW_GO(ROWS_MAX_M, GP_TILE, false);
    } else {
        if (low) RW_GO(ROWS_WIDE_M, 32, false);
        else if (nt_loads) RW_GO(ROWS_WIDE_M, GP_TILE, true);
        else RW_GO(ROWS_WIDE_M, GP_TILE, false);
    }
#undef RW_GO
}

void launch_rows(hipStream_t s, const double *Li, long Npad, const RowsX &rx, const KernParams &kp, const double *X, long N,
                 const double *alpha, int want_grad, double kss, double noise_add, const RowsAcq &aq, const RowsWork &w,
                 const PassReport &r, int nt_loads, const RowsMean &mf) {
    launch_rows_any(s, Li, Npad, rx, kp, X, N, alpha, want_grad, kss, noise_add, aq, w, r, nt_loads, false, mf);
}

// the forward launch alone: another kernel finishes the pass from w.wpart (es.hip)
void launch_rows_forward(hipStream_t s, const double *Li, long Npad, const RowsX &rx, const KernParams &kp, const double *X, long N,
                         const double *alpha, const RowsWork &w, int nt_loads) {
    launch_rows_any(s, Li, Npad, rx, kp, X, N, alpha, 0, 0.0, 0.0, RowsAcq{}, w, PassReport{}, nt_loads, true, RowsMean{0, nullptr, nullptr});
}

// the backward launch alone, over the w.wpart a forward launch of M locations left: w.bpart (and w.vpart), the instances launch_rows
// runs for that M and that matrix (qei.hip finishes the pass)
void launch_rows_backward(hipStream_t s, const double *Li, long Npad, int M, const RowsWork &w, int nt_loads) {
    const int nt = (int)(Npad / GP_TILE);
    const bool low = rows_block_height(nt) == 32;
#define RW_BK(MV, RB, NT)                                                                                                              \
    GP_LAUNCH((rows_backward_kernel<MV, RB, NT>), dim3((unsigned)rows_tiles(nt) * (GP_TILE / RB)), dim3(256), 0, s, Li, Npad, w.wpart, Npad, M, \
              w.bpart, w.vpart)
    if (M == 1) {
        if (low) RW_BK(1, 32, false);
        else if (nt_loads) RW_BK(1, GP_TILE, true);
        else RW_BK(1, GP_TILE, false);
    } else if (M <= ROWS_MAX_M) {
        if (low) RW_BK(ROWS_MAX_M, 32, false);
        else if (nt_loads) RW_BK(ROWS_MAX_M, GP_TILE, true);
        else RW_BK(ROWS_MAX_M, GP_TILE, false);
    } else {
        if (low) RW_BK(ROWS_WIDE_M, 32, false);
        else if (nt_loads) RW_BK(ROWS_WIDE_M, GP_TILE, true);
        else RW_BK(ROWS_WIDE_M, GP_TILE, false);
    }
#undef RW_BK
}

// ---- Li = (L^-T)^T: lower triangular, explicit zeros above the diagonal; and back -------------------------------------------------------
// mode 0: dst lower <- transpose of src upper;  mode 1: dst upper <- transpose of src lower.  32 x 32 LDS tiles.
__global__ __launch_bounds__(256) void transpose_tri_kernel(double *dst, const double *src, long n, int mode) {
    __shared__ double t[32][33];
    const int bx = blockIdx.x, by = blockIdx.y;   // destination tile (by, bx)
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const bool skip = mode == 0 ? bx > by : bx < by;   // wholly on the zero side
    if (!skip)
        for (int r = ty; r < 32; r += 8) t[r][tx] = src[((long)bx * 32 + r) * n + (long)by * 32 + tx];
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const long i = (long)by * 32 + r, j = (long)bx * 32 + tx;
        const bool keep = !skip && (mode == 0 ? j <= i : j >= i);
        dst[i * n + j] = keep ? t[tx][r] : 0.0;
    }
}
void launch_transpose_tri(hipStream_t s, double *dst, const double *src, long n, int mode) {
    dim3 grid((unsigned)(n / 32), (unsigned)(n / 32));
    GP_LAUNCH(transpose_tri_kernel, grid, dim3(256), 0, s, dst, src, n, mode);
}
