// Posterior function samples by pathwise conditioning (Wilson et al., ICML 2020): the kernels behind the gp_paths_* entries.
//
//     f_s(x) = amp sum_j Wt[s, j] cos(omega_j . x + phase_j)  +  sum_n k(x, X_n) V[s, n]
//
// Four kernels, all on operands padded with zeros to the 16 of v_mfma_f64_16x16x4_f64 (Spad rows of Wt and V, Fpad features):
//
//   paths_residual_kernel   R = Y - Phi(X) W - sd z: cos tiles of 16 features x 64 training rows in LDS, contracted with Wt on the
//                           matrix cores (the right-hand sides of the solve for V, api_paths.hip)
//   paths_table_kernel      every path over the candidate table: tiles of K(x_i, X_n), 32 training rows x 64 candidates, are formed
//                           in LDS and contracted with V on the matrix cores; then the feature term, tile by tile, into a second
//                           accumulator.  K(Xs, X) never exists in memory
//   paths_argbest_kernel    per path the best row of the table, two levels, the path as blockIdx.y
//   paths_rows_kernel       a handful of locations by value, each on a path of its own, value and gradient: one row / feature per
//                           thread, one partial per workgroup, the last workgroup to arrive adds them in order into the pinned block
//
// Operand maps of the instruction (lane l): A[row l & 15][k = l >> 4], B[k = l >> 4][col l & 15], D[row (l >> 4) + 4 e][col l & 15]
// for accumulator entry e.  Rows are paths, columns training rows (residual) or candidates (table): an output element is its own
// dot product, over n in tile order and j in index order, so its bits depend on no other path and no other column.
#include "gphip_internal.h"

#define PT_COLS 64          // columns (training rows / candidates) per workgroup: 16 per wave
#define PT_KN 32            // training rows per K tile of the table kernel
#define PT_PITCH 80         // doubles between two rows of an LDS tile of PT_COLS columns: rows k and k + 1 of a B fetch on other banks
#define PT_VPITCH 36        // ... of the V tile (PT_KN columns)
#define PT_NST (PATHS_MAX_SPAD / PATHS_MMA)

// omega_j . x + phase_j: from the phase on, the D products in dimension order, each fused
__device__ __forceinline__ double paths_arg(const double *om, const double *x, int D, double b) {
    double t = b;
    for (int d = 0; d < D; ++d) t = fma(om[d], x[d], t);
    return t;
}
__device__ __forceinline__ double paths_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// acc[st] += Wt-tile(st) x cos-tile for one tile of 16 features at j0 (cf: [16][PT_PITCH], this wave's 16 columns at c0)
__device__ __forceinline__ void paths_feature_mma(const PathsPrior &pp, int nst, int j0, const double *cf, int c0, int lane,
                                                  double4_t (&acc)[PT_NST]) {
    const int li = lane & 15, lg = lane >> 4;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        const double b = cf[(4 * kk + lg) * PT_PITCH + c0 + li];
#pragma unroll
        for (int st = 0; st < PT_NST; ++st)
            if (st < nst) {
                const double a = pp.Wt[(long)(st * PATHS_MMA + li) * pp.Fpad + j0 + 4 * kk + lg];
                acc[st] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[st], 0, 0, 0);
            }
    }
}
// the cos tile of 16 features at j0 over this workgroup's PT_COLS columns, whose raw inputs are xr [PT_COLS][D + 1] in LDS
__device__ __forceinline__ void paths_cos_tile(const PathsPrior &pp, int D, int j0, const double *xr, double *cf, int tid) {
    const int c = tid & 63, jg = __builtin_amdgcn_readfirstlane(tid >> 6);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = j0 + 4 * jg + q;   // < Fpad: the padding's frequencies and phases are zeros, its weights too
        cf[(4 * jg + q) * PT_PITCH + c] = cos(paths_arg(pp.omega + (long)j * D, xr + c * (D + 1), D, pp.phase[j]));
    }
}

__global__ __launch_bounds__(256) void paths_residual_kernel(PathsPrior pp, int S, int D, const double *X, const double *Y, long N,
                                                             double sd, double *R, long ldr) {
    extern __shared__ double lds[];
    double *xr = lds;                          // [PT_COLS][D + 1]
    double *cf = lds + PT_COLS * (D + 1);      // [16][PT_PITCH]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long n0 = (long)blockIdx.x * PT_COLS;
    for (int i = tid; i < PT_COLS * D; i += 256) {
        const int c = i / D, d = i % D;
        xr[c * (D + 1) + d] = (n0 + c < N) ? X[(n0 + c) * D + d] : 0.0;
    }
    const int nst = pp.Spad / PATHS_MMA;
    double4_t acc[PT_NST];
#pragma unroll
    for (int st = 0; st < PT_NST; ++st) acc[st] = double4_t{0.0, 0.0, 0.0, 0.0};
    for (int j0 = 0; j0 < pp.Fpad; j0 += PATHS_MMA) {
        __syncthreads();   // the tile's readers of the previous round are done (first round: xr is written)
        paths_cos_tile(pp, D, j0, xr, cf, tid);
        __syncthreads();
        paths_feature_mma(pp, nst, j0, cf, wave * 16, lane, acc);
    }
    const long n = n0 + wave * 16 + (lane & 15);
    if (n >= N) return;
    const double y = Y[n];
#pragma unroll
    for (int st = 0; st < PT_NST; ++st)
        if (st < nst)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int s = st * PATHS_MMA + (lane >> 4) + 4 * e;
                if (s < S) {
                    double *r = R + (long)s * ldr + n;
                    *r = fma(-sd, *r, fma(-pp.amp, acc[st][e], y));
                }
            }
}
void launch_paths_residual(hipStream_t s, const PathsPrior &pp, int S, int D, const double *X, const double *Y, long N, double sd,
                           double *R, long ldr) {
    const size_t shm = ((size_t)PT_COLS * (D + 1) + 16 * PT_PITCH) * sizeof(double);
    GP_LAUNCH(paths_residual_kernel, dim3((unsigned)((N + PT_COLS - 1) / PT_COLS)), dim3(256), shm, s, pp, S, D, X, Y, N, sd, R, ldr);
}

// ---- the table ---------------------------------------------------------------------------------------------------------------------------
// A workgroup takes PT_COLS candidates.  Bound by the exponentials and the fused differences of the K tile (M N (3 D + ~30)
// vector operations) beside 2 M N Spad flops on the matrix cores; X and V are re-read per workgroup from L2 (N (D + Spad) doubles).
// nsplit > 1: the training rows are cut into nsplit chunks of `chunk` rows (a multiple of PT_KN), blockIdx.y = chunk, and one more
// blockIdx.y takes the feature term; each writes its sums to part [nsplit + 1][S][M] and paths_table_sum_kernel adds them in
// chunk order.  nsplit = 1: one workgroup does it all and writes out itself.  Either way a sum's order is a function of (M, N).
__global__ __launch_bounds__(256) void paths_table_kernel(PathsPrior pp, int S, KernParams kp, const double *Xs, long M, const double *X,
                                                          long N, const double *V, long ldv, double y_mean, double y_std,
                                                          double *out, int nsplit, long chunk, double *part) {
    extern __shared__ double lds[];
    const int D = kp.D;
    double *xr = lds;                              // [PT_COLS][D + 1]: the candidates as given (the feature term's inputs)
    double *xc = xr + PT_COLS * (D + 1);           // [PT_COLS][D + 1]: ... over the lengthscales
    double *xt = xc + PT_COLS * (D + 1);           // [PT_KN][D]: a tile of training rows over the lengthscales
    double *ks = xt + PT_KN * D;                   // [PT_KN][PT_PITCH]: the K tile; then [16][PT_PITCH]: a cos tile
    double *vs = ks + PT_KN * PT_PITCH;            // [Spad][PT_VPITCH]: V of the tile's training rows
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lg = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long i0 = (long)blockIdx.x * PT_COLS;
    for (int i = tid; i < PT_COLS * D; i += 256) {
        const int c = i / D, d = i % D;
        const double x = (i0 + c < M) ? Xs[(i0 + c) * D + d] : 0.0;
        xr[c * (D + 1) + d] = x;
        xc[c * (D + 1) + d] = x / kp.ls[d];
    }
    const int nst = pp.Spad / PATHS_MMA;
    double4_t acc[PT_NST], accf[PT_NST];
#pragma unroll
    for (int st = 0; st < PT_NST; ++st) acc[st] = accf[st] = double4_t{0.0, 0.0, 0.0, 0.0};
    const int c = tid & 63, ng = wave;   // K tile: this thread's candidate and its 8 training rows ng * 8 ..
    const int y = (int)blockIdx.y;
    const bool do_k = nsplit == 1 || y < nsplit, do_f = nsplit == 1 || y == nsplit;   // (uniform over the workgroup)
    const long nbeg = nsplit == 1 ? 0 : (long)y * chunk, nend = do_k ? (nsplit == 1 ? N : min(N, nbeg + chunk)) : 0;
    for (long n0 = nbeg; n0 < nend; n0 += PT_KN) {
        __syncthreads();   // the previous tile's readers are done
        for (int i = tid; i < PT_KN * D; i += 256) {
            const int r = i / D, d = i % D;
            xt[i] = (n0 + r < N) ? X[(n0 + r) * D + d] / kp.ls[d] : 0.0;
        }
        for (int i = tid; i < pp.Spad * PT_KN; i += 256) {
            const int s = i / PT_KN, r = i % PT_KN;
            vs[s * PT_VPITCH + r] = (n0 + r < N) ? V[(long)s * ldv + n0 + r] : 0.0;
        }
        __syncthreads();
        double r2[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) r2[q] = 0.0;
        for (int d = 0; d < D; ++d) {
            const double x = xc[c * (D + 1) + d];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const double df = x - xt[(ng * 8 + q) * D + d];
                r2[q] = fma(df, df, r2[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < 8; ++q)
            ks[(ng * 8 + q) * PT_PITCH + c] = (n0 + ng * 8 + q < N) ? gp_k_of_r2(kp.kernel, kp.variance, r2[q]) : 0.0;
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < PT_KN / 4; ++kk) {
            const double b = ks[(4 * kk + lg) * PT_PITCH + wave * 16 + li];
#pragma unroll
            for (int st = 0; st < PT_NST; ++st)
                if (st < nst)
                    acc[st] = __builtin_amdgcn_mfma_f64_16x16x4f64(vs[(st * PATHS_MMA + li) * PT_VPITCH + 4 * kk + lg], b, acc[st], 0, 0, 0);
        }
    }
    for (int j0 = 0; do_f && j0 < pp.Fpad; j0 += PATHS_MMA) {
        __syncthreads();
        paths_cos_tile(pp, D, j0, xr, ks, tid);
        __syncthreads();
        paths_feature_mma(pp, nst, j0, ks, wave * 16, lane, accf);
    }
    const long i = i0 + wave * 16 + li;
    if (i >= M) return;
#pragma unroll
    for (int st = 0; st < PT_NST; ++st)
        if (st < nst)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int s = st * PATHS_MMA + lg + 4 * e;
                if (s >= S) continue;
                if (nsplit == 1) out[(long)s * M + i] = fma(y_std, fma(pp.amp, accf[st][e], acc[st][e]), y_mean);
                else part[((long)y * S + s) * M + i] = do_f ? accf[st][e] : acc[st][e];
            }
}
__global__ __launch_bounds__(256) void paths_table_sum_kernel(const double *part, long SM, int nsplit, double amp, double y_mean,
                                                              double y_std, double *out) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= SM) return;
    double k = 0.0;
    for (int y = 0; y < nsplit; ++y) k += part[(long)y * SM + e];
    out[e] = fma(y_std, fma(amp, part[(long)nsplit * SM + e], k), y_mean);
}
// chunks of the training rows for a table of M rows: enough workgroups to fill the chip, at least four K tiles each
int paths_table_split(long M, long N, long *chunk) {
    const long mb = (M + PT_COLS - 1) / PT_COLS, tiles = (N + PT_KN - 1) / PT_KN;
    long nsplit = std::max(1L, std::min(1024 / mb, tiles / 4));
    const long per = (tiles + nsplit - 1) / nsplit;
    nsplit = (tiles + per - 1) / per;
    *chunk = per * PT_KN;
    return (int)nsplit;
}
size_t paths_table_part_elems(long M, long N, int S) {
    long chunk;
    const int nsplit = paths_table_split(M, N, &chunk);
    return nsplit == 1 ? 0 : (size_t)(nsplit + 1) * S * M;
}
size_t paths_table_lds_bytes(int D, int Spad) {
    return ((size_t)2 * PT_COLS * (D + 1) + (size_t)PT_KN * D + PT_KN * PT_PITCH + (size_t)Spad * PT_VPITCH) * sizeof(double);
}
void launch_paths_table(hipStream_t s, const PathsPrior &pp, int S, const KernParams &kp, const double *Xs, long M, const double *X,
                        long N, const double *V, long ldv, double y_mean, double y_std, double *out, double *part) {
    long chunk;
    const int nsplit = paths_table_split(M, N, &chunk);
    const dim3 grid((unsigned)((M + PT_COLS - 1) / PT_COLS), nsplit == 1 ? 1 : nsplit + 1);
    GP_LAUNCH(paths_table_kernel, grid, dim3(256), paths_table_lds_bytes(kp.D, pp.Spad), s, pp, S, kp, Xs, M, X, N, V, ldv, y_mean, y_std,
              out, nsplit, chunk, part);
    if (nsplit > 1)
        GP_LAUNCH(paths_table_sum_kernel, dim3((unsigned)(((long)S * M + 255) / 256)), dim3(256), 0, s, (const double *)part, (long)S * M,
                  nsplit, pp.amp, y_mean, y_std, out);
}

// ---- per-path arg-best (NumPy's tie rule: the lowest index) ------------------------------------------------------------------------------
__device__ __forceinline__ void paths_better(double &v, long long &i, double v2, long long i2, int sense) {
    const bool better = (sense > 0) ? (v2 > v) : (v2 < v);
    if (better || (v2 == v && i2 < i)) {
        v = v2;
        i = i2;
    }
}
// level 0: block (b, s) over rows b 256 + tid, + gridDim.x 256, .. of x + s ldx; level 1: block (0, s) over the nb winners of path s
__global__ __launch_bounds__(256) void paths_argbest_kernel(const double *x, long ldx, long n, const long long *in_idx, int sense,
                                                            double *ov, long long *oi, long ldo) {
    __shared__ double sv[256];
    __shared__ long long si[256];
    const int tid = threadIdx.x;
    const long s = blockIdx.y;
    double v = (sense > 0) ? -INFINITY : INFINITY;
    long long bi = 0x7fffffffffffffffLL;
    for (long i = (long)blockIdx.x * 256 + tid; i < n; i += (long)gridDim.x * 256)
        paths_better(v, bi, x[s * ldx + i], in_idx ? in_idx[s * ldx + i] : (long long)i, sense);
    sv[tid] = v;
    si[tid] = bi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) paths_better(sv[tid], si[tid], sv[tid + o], si[tid + o], sense);
        __syncthreads();
    }
    if (tid == 0) {
        ov[s * ldo + blockIdx.x] = sv[0];
        oi[s * ldo + blockIdx.x] = si[0];
    }
}
void launch_paths_argbest(hipStream_t s, const double *tab, long M, int S, int sense, double *rv, long long *ri) {
    int nb = (int)std::min<long>(256, std::max<long>(1, (M + 255) / 256));
    GP_LAUNCH(paths_argbest_kernel, dim3(nb, S), dim3(256), 0, s, tab, M, M, (const long long *)nullptr, sense, rv + S, ri + S, 256L);
    GP_LAUNCH(paths_argbest_kernel, dim3(1, S), dim3(256), 0, s, (const double *)(rv + S), 256L, (long)nb, (const long long *)(ri + S),
              sense, rv, ri, 1L);
}

// ---- a handful of locations by value -----------------------------------------------------------------------------------------------------
// Workgroups 0 .. nkb - 1 take PATHS_ROWS_CH training rows each (one per thread), the rest PATHS_ROWS_CH features each.  Per
// location m: slot m (D + 1) the value's sum, slots m (D + 1) + 1 + d the gradient's.  A slot's partial is a fixed tree over the
// workgroup (six shuffle levels, then the four waves in order); the last workgroup to arrive adds the partials in workgroup order.
// Nothing in a location's arithmetic looks at M, at its slot or at another location: the same bits in any company.  Streams
// N (D + 1) + F (D + 2) doubles per location.
__global__ __launch_bounds__(256) void paths_rows_kernel(PathsPrior pp, RowsX rx, PathsPick pk, KernParams kp, const double *X, long N,
                                                         const double *V, long ldv, int want_grad, double y_mean, double y_std,
                                                         double *gpart, unsigned int *counter, unsigned int counter_base, double *out,
                                                         double ticket) {
    __shared__ double xs_s[ROWS_MAX_XS];
    __shared__ double sh[4][PATHS_ROWS_GROW];
    __shared__ int last_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int D = kp.D, M = rx.M, nq = want_grad ? D + 1 : 1, nval = M * (D + 1);
    const int nkb = (int)((N + PATHS_ROWS_CH - 1) / PATHS_ROWS_CH);
    if ((int)blockIdx.x < nkb) {
        for (int i = tid; i < M * D; i += 256) xs_s[i] = rx.xs[i] / kp.ls[i % D];
        __syncthreads();
        const long n = (long)blockIdx.x * PATHS_ROWS_CH + tid;
        const bool live = n < N;
        for (int m = 0; m < M; ++m) {
            double r2 = 0.0;
            if (live)
                for (int d = 0; d < D; ++d) {
                    const double df = xs_s[m * D + d] - X[n * D + d] / kp.ls[d];
                    r2 = fma(df, df, r2);
                }
            double kv, gv;
            gp_k_and_g(kp.kernel, kp.variance, r2, kv, gv);
            if (r2 == 0.0) gv = 0.0;   // invdist = 0 where the distance is exactly 0 (stationary.py:251-258)
            const double v = live ? V[(long)pk.path[m] * ldv + n] : 0.0;
            for (int q = 0; q < nq; ++q) {
                double t = 0.0;
                if (live) t = q == 0 ? kv * v : (gv * v) * (xs_s[m * D + q - 1] - X[n * D + q - 1] / kp.ls[q - 1]);
                t = paths_wave_sum(t);
                if (lane == 0) sh[wave][m * (D + 1) + q] = t;
            }
        }
    } else {
        for (int i = tid; i < M * D; i += 256) xs_s[i] = rx.xs[i];
        __syncthreads();
        const int j = ((int)blockIdx.x - nkb) * PATHS_ROWS_CH + tid;
        const bool live = j < pp.F;
        for (int m = 0; m < M; ++m) {
            double sn = 0.0, cs = 0.0, w = 0.0;
            if (live) {
                sincos(paths_arg(pp.omega + (long)j * D, xs_s + m * D, D, pp.phase[j]), &sn, &cs);
                w = pp.Wt[(long)pk.path[m] * pp.Fpad + j];
            }
            for (int q = 0; q < nq; ++q) {
                double t = 0.0;
                if (live) t = q == 0 ? w * cs : -(w * sn) * pp.omega[(long)j * D + q - 1];
                t = paths_wave_sum(t);
                if (lane == 0) sh[wave][m * (D + 1) + q] = t;
            }
        }
    }
    __syncthreads();
    if (tid < nval && tid % (D + 1) < nq)   // (a value-only call fills the values' slots alone)
        gpart[(long)blockIdx.x * PATHS_ROWS_GROW + tid] = ((sh[0][tid] + sh[1][tid]) + sh[2][tid]) + sh[3][tid];
    __threadfence();
    __syncthreads();
    if (tid == 0) last_s = (atomicAdd(counter, 1u) - counter_base == gridDim.x - 1) ? 1 : 0;   // (unsigned: wraps with the base)
    __syncthreads();
    if (!last_s) return;
    __threadfence();
    if (tid < nval) {
        const int m = tid / (D + 1), q = tid % (D + 1);
        if (q < nq) {
            double sk = 0.0, sf = 0.0;
            for (int b = 0; b < nkb; ++b) sk += gpart[(long)b * PATHS_ROWS_GROW + tid];
            for (int b = nkb; b < (int)gridDim.x; ++b) sf += gpart[(long)b * PATHS_ROWS_GROW + tid];
            if (q == 0) out[m] = fma(y_std, fma(pp.amp, sf, sk), y_mean);
            else out[PATHS_ROWS_M + m * D + q - 1] = y_std * fma(pp.amp, sf, sk / kp.ls[q - 1]);   // (x - x') / l^2 = scaled difference / l
        }
    }
    __syncthreads();
    if (tid == 0) out[ROWS_OUT_DOUBLES] = ticket;
}
void launch_paths_rows(hipStream_t s, const PathsPrior &pp, const RowsX &rx, const PathsPick &pk, const KernParams &kp, const double *X,
                       long N, const double *V, long ldv, int want_grad, double y_mean, double y_std, double *gpart,
                       const PassReport &r) {
    GP_LAUNCH(paths_rows_kernel, dim3(paths_rows_grid(N, pp.F)), dim3(256), 0, s, pp, rx, pk, kp, X, N, V, ldv, want_grad, y_mean, y_std,
              gpart, r.counter, r.base, r.out, r.ticket);
}
