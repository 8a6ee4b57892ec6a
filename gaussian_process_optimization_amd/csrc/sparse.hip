// Kernels of the sparse GP (variational DTC): the weighted-gradient pass over the N x Mz cross-covariance block, the
// posterior reduction, and the small dense helpers of the Mz x Mz algebra (api_sparse.hip composes them with the GEMM,
// the tile Cholesky and the K-build launchers).
//
// Reference: SparseGP._update_gradients (GPy/GPy/core/sparse_gp.py:108-118) calls, for the certain-input case,
//   kern.update_gradients_full(dL_dKnm, X, Z), kern.update_gradients_full(dL_dKmm, Z, None)        (stationary.py:218-238)
//   kern.gradients_X(dL_dKmm, Z) + kern.gradients_X(dL_dKnm.T, Z, X)                               (stationary.py:336-352)
// with dL_dKnm = beta Y C^T + 2 beta Kfu E (var_dtc.py:218-234).  The reference makes D passes over N x Mz temporaries for each
// of them.  Here ONE pass regenerates r, k and g(r) = dK_dr / r from the scaled inputs and produces, for every inducing row m,
//   sum_n W[n, m] k,   sum_n W[n, m] g d_q   (-> dZ[m, q]),   sum_n W[n, m] g d_q^2   (-> the lengthscale sums),
// d_q = (z_mq - x_nq) / l_q.  It is the rectangular sibling of gradx_tile_kernel (gradx.hip): one lane per inducing row m, the
// data columns n streamed in 128-tiles with x_n / l and y_n staged in LDS, W[n, m] read with m contiguous (the 64 lanes of a wave
// load 512 contiguous bytes per n), the y . C term of the weight added on the fly, and every sum kept in its lane's registers.
// r^2 == 0 adds exactly 0 to the d_q sums (gp_k_and_g and the explicit select below), as _inv_dist does (stationary.py:251-258):
// with Z a subset of X coincident pairs are the norm.
//
// "Square" use (the Kmm part): columns := Z, W := dL_dKmm, P = 0 -- the same kernel; the factor 2 of gradients_X's tmp + tmp.T
// is applied by the summing kernel (zfac).
#include "gphip_internal.h"
#include "../../include/gphip.h"
#include <cstring>

#define GCH GP_GRAD_CH
#define SP_H 2                        // lanes per inducing row: each takes a half (64 columns) of every column tile
#define SP_CHUNK 4                    // column tiles per workgroup
#define SP_THREADS (SP_H * GP_TILE)
#define SP_NACC (1 + 2 * GCH)         // [0] sum W k, [1 + q] sum W g d_q, [1 + GCH + q] sum W g d_q^2

// Summation order of an inducing row, fixed by these constants alone (never by the grid): a lane adds its 64 columns of each of
// the chunk's column tiles in ascending column order; the row's two lanes are added h0 + h1; the summing kernels add the chunks
// in ascending order (dZ) or deal (chunk, row) pairs over 1024 threads in index order and add the threads as a fixed tree (the
// hyper-parameter sums).
// partial[(chunk * SP_NACC + a) * Mzpad + m]
template <int FP>
__device__ __forceinline__ void sparse_grad_tile_body(const double *Z, long Mz, long Mzpad, const double *Xc, long Nc, const KernParams &kp,
                                                      int d0, const double *Y, int P, const double *C, long ldc, double ybeta,
                                                      const double *Wt, long ldw, double wscale, double *partial) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int D = kp.D;
    double *zi = sm;                        // [D][128]
    double *xj = zi + (long)D * GP_TILE;    // [D][128]
    double *yj = xj + (long)D * GP_TILE;    // [P][128]
    const int tid = threadIdx.x;
    const int r = tid & (GP_TILE - 1), h = tid >> 7;
    const int tm = blockIdx.x;
    const int ntc = (int)((Nc + GP_TILE - 1) / GP_TILE);
    const int tn0 = (int)blockIdx.y * SP_CHUNK, tn1 = min(tn0 + SP_CHUNK, ntc);
    const long gm = (long)tm * GP_TILE + r;   // < Mzpad

    for (int idx = tid; idx < GP_TILE * D; idx += SP_THREADS) {
        const int rr = idx / D, d = idx - rr * D;
        const long g = (long)tm * GP_TILE + rr;
        zi[d * GP_TILE + rr] = (g < Mz) ? Z[g * D + d] / kp.ls[d] : 0.0;
    }
    double cm[GP_SPARSE_GRAD_MAX_P];
#pragma unroll
    for (int p = 0; p < GP_SPARSE_GRAD_MAX_P; ++p) cm[p] = (p < P && gm < Mz) ? C[(long)p * ldc + gm] : 0.0;

    double acck = 0.0, accz[GCH], accl[GCH], xq[GCH];
#pragma unroll
    for (int q = 0; q < GCH; ++q) accz[q] = accl[q] = xq[q] = 0.0;

    for (int tn = tn0; tn < tn1; ++tn) {
        __syncthreads();   // the previous column tile is consumed (first trip: orders the row staging above)
        for (int idx = tid; idx < GP_TILE * D; idx += SP_THREADS) {
            const int rr = idx / D, d = idx - rr * D;
            const long g = (long)tn * GP_TILE + rr;
            xj[d * GP_TILE + rr] = (g < Nc) ? Xc[g * D + d] / kp.ls[d] : 0.0;
        }
        for (int idx = tid; idx < GP_TILE * P; idx += SP_THREADS) {
            const int rr = idx / P, p = idx - rr * P;
            const long g = (long)tn * GP_TILE + rr;
            yj[p * GP_TILE + rr] = (g < Nc) ? Y[g * P + p] : 0.0;
        }
        __syncthreads();
        if (tn == tn0) {
#pragma unroll
            for (int q = 0; q < GCH; ++q) xq[q] = (d0 + q < D) ? zi[(d0 + q) * GP_TILE + r] : 0.0;
        }
        const int c0 = h * (GP_TILE / SP_H);
        for (int cc = 0; cc < GP_TILE / SP_H; ++cc) {
            const int c = c0 + cc;
            const long gj = (long)tn * GP_TILE + c;
            if (gj >= Nc) break;                                 // padding columns contribute nothing (uniform across the wave)
            double w = wscale * Wt[gj * ldw + gm];               // gm < Mzpad = ldw: inside the matrix for padding rows too
            if (P > 0) {
                double yc = 0.0;
#pragma unroll
                for (int p = 0; p < GP_SPARSE_GRAD_MAX_P; ++p)
                    if (p < P) yc = fma(yj[p * GP_TILE + c], cm[p], yc);
                w = fma(ybeta, yc, w);
            }
            double s = 0.0;
            for (int d = 0; d < D; ++d) {
                const double df = zi[d * GP_TILE + r] - xj[d * GP_TILE + c];
                s = fma(df, df, s);
            }
            double kv, gv;
            gp_k_and_g_pair<FP>(kp.kernel, kp.variance, s, kv, gv);
            acck = fma(w, kv, acck);
            const double t = (s == 0.0) ? 0.0 : w * gv;          // _inv_dist is 0 where the distance is 0
#pragma unroll
            for (int q = 0; q < GCH; ++q)
                if (d0 + q < D) {
                    const double dq = xq[q] - xj[(d0 + q) * GP_TILE + c];
                    const double tq = t * dq;
                    accz[q] += tq;
                    accl[q] = fma(tq, dq, accl[q]);
                }
        }
    }
    // the row's lanes, in fixed order (the staging area is free: at least SP_NACC * 128 doubles, see launch_sparse_grad)
    __syncthreads();
    double *red = sm;   // [SP_NACC][128]
    if (h == 1) {
        red[r] = acck;
#pragma unroll
        for (int q = 0; q < GCH; ++q) {
            red[(1 + q) * GP_TILE + r] = accz[q];
            red[(1 + GCH + q) * GP_TILE + r] = accl[q];
        }
    }
    __syncthreads();
    if (h == 0) {
        double *out = partial + (long)blockIdx.y * SP_NACC * Mzpad + gm;
        out[0] = acck + red[r];
#pragma unroll
        for (int q = 0; q < GCH; ++q) {
            out[(long)(1 + q) * Mzpad] = accz[q] + red[(1 + q) * GP_TILE + r];
            out[(long)(1 + GCH + q) * Mzpad] = accl[q] + red[(1 + GCH + q) * GP_TILE + r];
        }
    }
}

template <int FP>
__global__ __launch_bounds__(SP_THREADS) void sparse_grad_tile_kernel(const double *Z, long Mz, long Mzpad, const double *Xc, long Nc,
                                                                      KernParams kp, int d0, const double *Y, int P, const double *C,
                                                                      long ldc, double ybeta, const double *Wt, long ldw, double wscale,
                                                                      double *partial) {
    sparse_grad_tile_body<FP>(Z, Mz, Mzpad, Xc, Nc, kp, d0, Y, P, C, ldc, ybeta, Wt, ldw, wscale, partial);
}
// member z = blockIdx.z of a batch (gp_sparse_fit_grad_batch): rows Z + z sZ, columns Xc + z sXc (0: the shared data), parameters
// kpt[z] (device table), woodbury rows C + z sC, weights Wt + z sW, the scales ybeta_tab[z] / wscale_tab[z] (a null table: the
// value given) and slabs at partial + z sP.  The body is the single problem's: a member's sums are added in the order the
// constants above fix.
template <int FP>
__global__ __launch_bounds__(SP_THREADS) void sparse_grad_tile_batch_kernel(const double *Z, long sZ, long Mz, long Mzpad, const double *Xc,
                                                                            long sXc, long Nc, const KernParams *kpt, int d0,
                                                                            const double *Y, int P, const double *C, long sC, long ldc,
                                                                            double ybeta, const double *ybeta_tab, const double *Wt,
                                                                            long sW, long ldw, double wscale, const double *wscale_tab,
                                                                            double *partial, long sP) {
    const long z = blockIdx.z;
    sparse_grad_tile_body<FP>(Z + z * sZ, Mz, Mzpad, Xc + z * sXc, Nc, kpt[z], d0, Y, P, C + z * sC, ldc,
                              ybeta_tab ? ybeta_tab[z] : ybeta, Wt + z * sW, ldw, wscale_tab ? wscale_tab[z] : wscale, partial + z * sP);
}

// dZ[m, d0 + q] = zfac (sum over the chunks, ascending) / l_q for m < Mz: (z - x) / l^2 = scaled difference / l
// (member z = blockIdx.z: slabs at partial + z sP, lengthscales of kpt[z], rows at dZ + z sD; a null kpt: one problem, kp's)
__global__ __launch_bounds__(256) void sparse_dz_sum_kernel(const double *partial, long Mz, long Mzpad, int nchunk, KernParams kp, int d0,
                                                            double zfac, double *dZ, long sP, long sD, const KernParams *kpt) {
    const long m = (long)blockIdx.x * 256 + threadIdx.x;   // adjacent lanes take adjacent rows: the slabs are read coalesced
    const int q = blockIdx.y;
    const long z = blockIdx.z;
    if (m >= Mz || d0 + q >= kp.D) return;
    partial += z * sP;
    double s = 0.0;
    for (int k = 0; k < nchunk; ++k) s += partial[((long)k * SP_NACC + 1 + q) * Mzpad + m];
    const double l = kpt ? kpt[z].ls[d0 + q] : kp.ls[d0 + q];
    dZ[z * sD + m * kp.D + d0 + q] = zfac * s / l;
}

__device__ __forceinline__ double sp_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}
// sum over the workgroup's NT threads, lane 0 of each wave in wave order; every thread gets it
template <int NT>
__device__ __forceinline__ double sp_block_sum(double v, double *sh) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    v = sp_wave_sum(v);
    if (lane == 0) sh[wv] = v;
    __syncthreads();
    double r = 0.0;
    for (int i = 0; i < NT / 64; ++i) r += sh[i];
    __syncthreads();
    return r;
}

// out[0] = sum W k, out[1 + q] = sum W g d_q^2 of the pass, over the chunks and the rows m < Mz: one workgroup per sum
// (member z = blockIdx.y: slabs at partial + z sP, sums at out + z sO)
__global__ __launch_bounds__(1024) void sparse_hyper_sum_kernel(const double *partial, long Mz, long Mzpad, int nchunk, int D, int d0,
                                                                double *out, long sP, long sO) {
    __shared__ double sh[16];
    const int a = blockIdx.x;
    partial += (long)blockIdx.y * sP;
    out += (long)blockIdx.y * sO;
    const int src = a == 0 ? 0 : GCH + a;
    double s = 0.0;
    if (a == 0 || d0 + a - 1 < D)
        for (long e = threadIdx.x; e < (long)nchunk * Mz; e += 1024) {
            const long k = e / Mz, m = e - k * Mz;
            s += partial[(k * SP_NACC + src) * Mzpad + m];
        }
    s = sp_block_sum<1024>(s, sh);
    if (threadIdx.x == 0) out[a] = s;
}

long sparse_grad_partial_elems(long Mzpad, long Nc) {
    const long ntc = (Nc + GP_TILE - 1) / GP_TILE;
    return (ntc + SP_CHUNK - 1) / SP_CHUNK * SP_NACC * Mzpad;
}

// LDS of one workgroup of sparse_grad_tile_kernel in bytes (all of it dynamic): the inducing rows' tile, the column tile of the
// inputs and of the P targets, and never less than the reduction's SP_NACC rows of 128 (gp_sparse_fit_grad holds it against the
// device's limit before anything is launched)
size_t sparse_grad_lds_bytes(int D, int P) {
    const size_t stage = ((size_t)2 * D + P) * GP_TILE * sizeof(double);
    return std::max(stage, (size_t)SP_NACC * GP_TILE * sizeof(double));
}

void launch_sparse_grad(hipStream_t s, const double *Z, long Mz, long Mzpad, const double *Xc, long Nc, const KernParams &kp,
                        const double *Y, int P, const double *C, long ldc, double ybeta, const double *Wt, long ldw, double wscale,
                        double *partial, double zfac, double *dZ, double *hyper, const SparseGradMembers *mb) {
    const int ntz = (int)(Mzpad / GP_TILE);
    const int ntc = (int)((Nc + GP_TILE - 1) / GP_TILE);
    const int nchunk = (ntc + SP_CHUNK - 1) / SP_CHUNK;
    const size_t shm = sparse_grad_lds_bytes(kp.D, P);
    const int fp = GP_FAMILY_PAIR(kp.kernel);
    const unsigned nb = mb ? (unsigned)mb->nb : 1u;
    const SparseGradMembers one{};
    const SparseGradMembers &m = mb ? *mb : one;
    int pass = 0;
    for (int d0 = 0; d0 < kp.D; d0 += GCH, ++pass) {
        if (mb) {   // kernel family, D and P -- what picks the instance and the LDS size -- are the same for every member
            const dim3 grid((unsigned)ntz, (unsigned)nchunk, nb);
            if (fp)
                GP_LAUNCH(sparse_grad_tile_batch_kernel<1>, grid, dim3(SP_THREADS), shm, s, Z, m.sZ, Mz, Mzpad, Xc, m.sXc, Nc, m.kpt, d0, Y,
                          P, C, m.sC, ldc, ybeta, m.ybeta_tab, Wt, m.sW, ldw, wscale, m.wscale_tab, partial, m.sP);
            else
                GP_LAUNCH(sparse_grad_tile_batch_kernel<0>, grid, dim3(SP_THREADS), shm, s, Z, m.sZ, Mz, Mzpad, Xc, m.sXc, Nc, m.kpt, d0, Y,
                          P, C, m.sC, ldc, ybeta, m.ybeta_tab, Wt, m.sW, ldw, wscale, m.wscale_tab, partial, m.sP);
        } else if (fp)
            GP_LAUNCH(sparse_grad_tile_kernel<1>, dim3((unsigned)ntz, (unsigned)nchunk), dim3(SP_THREADS), shm, s, Z, Mz, Mzpad, Xc, Nc,
                      kp, d0, Y, P, C, ldc, ybeta, Wt, ldw, wscale, partial);
        else
            GP_LAUNCH(sparse_grad_tile_kernel<0>, dim3((unsigned)ntz, (unsigned)nchunk), dim3(SP_THREADS), shm, s, Z, Mz, Mzpad, Xc, Nc,
                      kp, d0, Y, P, C, ldc, ybeta, Wt, ldw, wscale, partial);
        GP_LAUNCH(sparse_dz_sum_kernel, dim3((unsigned)((Mz + 255) / 256), GCH, nb), dim3(256), 0, s, partial, Mz, Mzpad, nchunk, kp, d0,
                  zfac, dZ, m.sP, m.sDZ, m.kpt);
        GP_LAUNCH(sparse_hyper_sum_kernel, dim3(GP_SPARSE_NH, nb), dim3(1024), 0, s, partial, Mz, Mzpad, nchunk, kp.D, d0,
                  hyper + (long)pass * GP_SPARSE_NH, m.sP, m.sH);
    }
}

// ---- the small dense helpers of the Mz x Mz algebra (n = Mzpad, leading dimension n) -----------------------------------------
// Each helper takes nb members in one launch (the member is the last grid index): member z's operands at base + z stride, its
// per-member coefficient from a device table where one is given (null: the value in the arguments, for every member).  One
// member with zero strides and no tables is the single problem: the same body, the same bits.
// out = a X + b Y + c I  (Y may be null)
__global__ __launch_bounds__(256) void sparse_lincomb_kernel(double *out, const double *X, double a, const double *Y, double b, double c,
                                                             long n, long sO, long sX, long sY, const double *a_tab, const double *b_tab) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * n) return;
    const long z = blockIdx.y;
    out += z * sO;
    X += z * sX;
    if (a_tab) a = a_tab[z];
    if (b_tab) b = b_tab[z];
    const long i = e / n, j = e - i * n;
    double v = a * X[e];
    if (Y) v = fma(b, Y[z * sY + e], v);
    out[e] = v + (i == j ? c : 0.0);
}
void launch_sparse_lincomb(hipStream_t s, double *out, const double *X, double a, const double *Y, double b, double c, long n, int nb,
                           long sO, long sX, long sY, const double *a_tab, const double *b_tab) {
    GP_LAUNCH(sparse_lincomb_kernel, dim3((unsigned)((n * n + 255) / 256), (unsigned)nb), dim3(256), 0, s, out, X, a, Y, b, c, n, sO, sX,
              sY, a_tab, b_tab);
}
// out = c I + sum_p v_p v_p^T,  v_p = V + p ldv (n entries)
__global__ __launch_bounds__(256) void sparse_outer_kernel(double *out, const double *V, long ldv, int P, double c, long n, long sO,
                                                           long sV) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * n) return;
    out += (long)blockIdx.y * sO;
    V += (long)blockIdx.y * sV;
    const long i = e / n, j = e - i * n;
    double v = 0.0;
    for (int p = 0; p < P; ++p) v = fma(V[p * ldv + i], V[p * ldv + j], v);
    out[e] = v + (i == j ? c : 0.0);
}
void launch_sparse_outer(hipStream_t s, double *out, const double *V, long ldv, int P, double c, long n, int nb, long sO, long sV) {
    GP_LAUNCH(sparse_outer_kernel, dim3((unsigned)((n * n + 255) / 256), (unsigned)nb), dim3(256), 0, s, out, V, ldv, P, c, n, sO, sV);
}
// out[p ldo + i] = scale sum_{k < K} M[i ldm + k] v[p vsp + k vsk]   for i < rows, p < P: one workgroup per (i, p), thread t
// takes k = t, t + 256, ... in order, the threads added as a fixed tree
__global__ __launch_bounds__(256) void sparse_thin_kernel(const double *M, long ldm, long K, const double *v, long vsp, long vsk,
                                                          double scale, double *out, long ldo, long sM, long sv, long so,
                                                          const double *scale_tab) {
    __shared__ double sh[4];
    const long i = blockIdx.x, p = blockIdx.y, z = blockIdx.z;
    M += z * sM;
    v += z * sv;
    if (scale_tab) scale = scale_tab[z];
    double s = 0.0;
    for (long k = threadIdx.x; k < K; k += 256) s = fma(M[i * ldm + k], v[p * vsp + k * vsk], s);
    s = sp_block_sum<256>(s, sh);
    if (threadIdx.x == 0) out[z * so + p * ldo + i] = scale * s;
}
void launch_sparse_thin(hipStream_t s, const double *M, long ldm, long rows, long K, const double *v, long vsp, long vsk, int P,
                        double scale, double *out, long ldo, int nb, long sM, long sv, long so, const double *scale_tab) {
    GP_LAUNCH(sparse_thin_kernel, dim3((unsigned)rows, (unsigned)P, (unsigned)nb), dim3(256), 0, s, M, ldm, K, v, vsp, vsk, scale, out,
              ldo, sM, sv, so, scale_tab);
}
// out[0] = sum Y^2, out[1] = trace(VVt) (i < Mz), out[2] = sum_p |c_p|^2 (data_fit), out[3] = sum VVt o Dm (n x n; VVt is zero in
// the padding): one workgroup each
__global__ __launch_bounds__(1024) void sparse_scalars_kernel(const double *Y, long NP, const double *VVt, const double *Dm, long Mz, long n,
                                                              const double *c1, int P, double *out, long sT, long sc, long so) {
    __shared__ double sh[16];
    double s = 0.0;
    const int t = threadIdx.x;
    const long z = blockIdx.y;
    VVt += z * sT;
    Dm += z * sT;
    c1 += z * sc;
    out += z * so;
    if (blockIdx.x == 0) {
        for (long e = t; e < NP; e += 1024) s = fma(Y[e], Y[e], s);
    } else if (blockIdx.x == 1) {
        for (long i = t; i < Mz; i += 1024) s += VVt[i * n + i];
    } else if (blockIdx.x == 2) {
        for (long e = t; e < (long)P * n; e += 1024) s = fma(c1[e], c1[e], s);
    } else {
        for (long e = t; e < n * n; e += 1024) s = fma(VVt[e], Dm[e], s);
    }
    s = sp_block_sum<1024>(s, sh);
    if (t == 0) out[blockIdx.x] = s;
}
void launch_sparse_scalars(hipStream_t s, const double *Y, long NP, const double *VVt, const double *Dm, long Mz, long n, const double *c1,
                           int P, double *out, int nb, long sT, long sc, long so) {
    GP_LAUNCH(sparse_scalars_kernel, dim3(4, (unsigned)nb), dim3(1024), 0, s, Y, NP, VVt, Dm, Mz, n, c1, P, out, sT, sc, so);
}

// ---- posterior reduction (posterior.py:225-248) -----------------------------------------------------------------------------
// mean[c, p] = sum_m Kx[c, m] w_p[m];  var[c] = max(kss - sum_m Bt[c, m] Kx[c, m], 1e-15) (+ noise_add).  One workgroup per
// candidate row: thread t takes m = t, t + 256, ... in order, the threads added as a fixed tree -- a row's result depends on
// nothing but its own row of Kx and Bt.
__global__ __launch_bounds__(256) void sparse_predict_reduce_kernel(const double *Kx, const double *Bt, long ld, long Mz, const double *w,
                                                                    long ldw, int P, double kss, double noise_add, double *mean,
                                                                    double *var) {
    __shared__ double sh[4];
    const long c = blockIdx.x;
    const double *kx = Kx + c * ld, *bt = Bt + c * ld;
    double s = 0.0;
    for (long m = threadIdx.x; m < Mz; m += 256) s = fma(bt[m], kx[m], s);
    s = sp_block_sum<256>(s, sh);
    if (threadIdx.x == 0) var[c] = fmax(kss - s, 1e-15) + noise_add;
    for (int p = 0; p < P; ++p) {
        double a = 0.0;
        for (long m = threadIdx.x; m < Mz; m += 256) a = fma(kx[m], w[p * ldw + m], a);
        a = sp_block_sum<256>(a, sh);
        if (threadIdx.x == 0) mean[c * P + p] = a;
    }
}
void launch_sparse_predict_reduce(hipStream_t s, const double *Kx, const double *Bt, long ld, long M, long Mz, const double *w, long ldw,
                                  int P, double kss, double noise_add, double *mean, double *var) {
    GP_LAUNCH(sparse_predict_reduce_kernel, dim3((unsigned)M), dim3(256), 0, s, Kx, Bt, ld, Mz, w, ldw, P, kss, noise_add, mean, var);
}

// out[0] = min v[0 .. n)
__global__ __launch_bounds__(1024) void sparse_min_kernel(const double *v, long n, double *out) {
    __shared__ double sh[1024];
    double m = INFINITY;
    for (long i = threadIdx.x; i < n; i += 1024) m = fmin(m, v[i]);
    sh[threadIdx.x] = m;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] = fmin(sh[threadIdx.x], sh[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sh[0];
}
void launch_sparse_min(hipStream_t s, const double *v, long n, double *out) {
    GP_LAUNCH(sparse_min_kernel, dim3(1), dim3(1024), 0, s, v, n, out);
}
