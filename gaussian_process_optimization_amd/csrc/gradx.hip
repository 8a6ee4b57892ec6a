// Input-side kernels of the input-warped GP: the LML gradient with respect to the training inputs, and the Kumaraswamy
// warp of a resident candidate table.
//
// Reference: InputWarpedGP.parameters_changed (GPy/GPy/models/input_warped_gp.py:94-103) calls
// kern.gradients_X(dL_dK, X) with X2 = None: Stationary.gradients_X (GPy/GPy/kern/src/stationary.py:336-352) with
// tmp + tmp.T (dL_dK is symmetric), _inv_dist (:251-258), dL_dK = 0.5 (alpha alpha^T - P Ky^-1)
// (exact_gaussian_inference.py:70); KumarWarping.f (GPy/GPy/util/input_warping_functions.py:179-200).
//
// The reference makes D passes over N x N temporaries.  Here ONE pass over Ky^-1 regenerates r and g(r) from the scaled
// inputs (staged in LDS) and produces every row's GCH sums:
//   dL_dX[i, q] = (1 / l_q) sum_{j != i} (sum_p alpha_pi alpha_pj - P Wi_ij) g(r_ij) (x_iq - x_jq) / l_q
// Mapping: one lane per row i.  Ky^-1 holds both triangles after the potri-equivalent, so the lane reads Wi[j, i] in place
// of Wi[i, j]: the 64 lanes of a wave load 512 contiguous bytes for every column j, x_j and alpha_j are LDS broadcasts, and
// the row's sums never leave its lane's registers.  Every element of Ky^-1 is read exactly once.
#include "gphip_internal.h"
#include "../../include/gphip.h"
#include <cstring>

#define GCH GP_GRAD_CH       // dimensions per pass (accumulators stay in registers)
#define GX_H 2               // lanes per row: each takes a half (64 columns) of every column tile
#define GX_CHUNK 4           // column tiles per workgroup
#define GX_THREADS (GX_H * GP_TILE)

// Summation order of a row, fixed by these constants alone (never by the grid): a lane adds its 32 columns of each of the
// chunk's column tiles in ascending column order; the row's two lanes are added h0 + h1; gradx_sum_kernel adds
// the chunks in ascending order.
// partial[(chunk * Npad + i) * GCH + q]
// MEMBERS = 1 (gp_fit_grad_x_batch): member z = blockIdx.z with inputs X + z sX, parameters kpt[z] (device table; kp1 is not
// read), alpha + z sV, Ky^-1 at Wi + z sW, partials at partial + z sP; the grid's x and y are the single launch's, so a member's
// row sums are added in the order the constants above fix.  MEMBERS = 0: one problem, parameters kp1 by value (kpt and the
// strides are not read).  One template and not a body with a _batch twin: with the body in a function of its own the
// single-member instances took 147 / 146 VGPRs instead of 137 / 135 (same occupancy step, but the figures DESIGN.md quotes);
// this form keeps all four instances at 137 / 135 with no scratch.
template <int FP, int MEMBERS>
__global__ __launch_bounds__(GX_THREADS) void gradx_tile_kernel(const double *X, long sX, long N, long Npad, KernParams kp1,
                                                                const KernParams *kpt, int d0, const double *alpha, long sV,
                                                                long lda_, int P, const double *Wi, long sW, long ldw,
                                                                double *partial, long sP) {
    const KernParams &kp = MEMBERS ? kpt[blockIdx.z] : kp1;
    if (MEMBERS) {
        const long z = blockIdx.z;
        X += z * sX;
        alpha += z * sV;
        Wi += z * sW;
        partial += z * sP;
    }
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int D = kp.D;
    double *xi = sm;                        // [D][128]
    double *xj = xi + (long)D * GP_TILE;    // [D][128]
    double *ai = xj + (long)D * GP_TILE;    // [P][128]
    double *aj = ai + (long)P * GP_TILE;    // [P][128]
    const int tid = threadIdx.x;
    const int r = tid & (GP_TILE - 1), h = tid >> 7;
    const int tm = blockIdx.x;
    const int nt = (int)(Npad / GP_TILE);
    const int tn0 = (int)blockIdx.y * GX_CHUNK, tn1 = min(tn0 + GX_CHUNK, nt);
    const long gi = (long)tm * GP_TILE + r;

    for (int idx = tid; idx < GP_TILE * D; idx += GX_THREADS) {
        const int rr = idx / D, d = idx - rr * D;
        const long g = (long)tm * GP_TILE + rr;
        xi[d * GP_TILE + rr] = (g < N) ? X[g * D + d] / kp.ls[d] : 0.0;
    }
    for (int idx = tid; idx < GP_TILE * P; idx += GX_THREADS) {
        const int p = idx / GP_TILE, rr = idx - p * GP_TILE;
        const long g = (long)tm * GP_TILE + rr;
        ai[idx] = (g < N) ? alpha[p * lda_ + g] : 0.0;
    }

    double acc[GCH], xq[GCH];
#pragma unroll
    for (int q = 0; q < GCH; ++q) acc[q] = 0.0;

    for (int tn = tn0; tn < tn1; ++tn) {
        __syncthreads();   // the previous column tile is consumed (first trip: orders the row staging above)
        for (int idx = tid; idx < GP_TILE * D; idx += GX_THREADS) {
            const int rr = idx / D, d = idx - rr * D;
            const long g = (long)tn * GP_TILE + rr;
            xj[d * GP_TILE + rr] = (g < N) ? X[g * D + d] / kp.ls[d] : 0.0;
        }
        for (int idx = tid; idx < GP_TILE * P; idx += GX_THREADS) {
            const int p = idx / GP_TILE, rr = idx - p * GP_TILE;
            const long g = (long)tn * GP_TILE + rr;
            aj[idx] = (g < N) ? alpha[p * lda_ + g] : 0.0;
        }
        __syncthreads();
        if (tn == tn0) {
#pragma unroll
            for (int q = 0; q < GCH; ++q) xq[q] = (d0 + q < D) ? xi[(d0 + q) * GP_TILE + r] : 0.0;
        }
        const int c0 = h * (GP_TILE / GX_H);
        for (int cc = 0; cc < GP_TILE / GX_H; ++cc) {
            const int c = c0 + cc;
            const long gj = (long)tn * GP_TILE + c;
            if (gj >= N) break;                                  // padding columns contribute nothing (uniform across the wave)
            const double w = Wi[gj * ldw + gi];                  // = Wi[gi, gj]; gi < Npad = ldw: inside the matrix for padding rows too
            double s = 0.0;
            for (int d = 0; d < D; ++d) {
                const double df = xi[d * GP_TILE + r] - xj[d * GP_TILE + c];
                s = fma(df, df, s);
            }
            double aa = 0.0;
            for (int p = 0; p < P; ++p) aa = fma(ai[p * GP_TILE + r], aj[p * GP_TILE + c], aa);
            double kv, gv;
            gp_k_and_g_pair<FP>(kp.kernel, kp.variance, s, kv, gv);
            // 2 dL_dK_ij g(r_ij); _inv_dist is 0 where the distance is 0 (stationary.py:251-258): the diagonal and coincident points
            const double t = (s == 0.0) ? 0.0 : gv * (aa - (double)P * w);
#pragma unroll
            for (int q = 0; q < GCH; ++q)
                if (d0 + q < D) acc[q] = fma(t, xq[q] - xj[(d0 + q) * GP_TILE + c], acc[q]);
        }
    }
    // the row's lanes, in fixed order (the staging area is free: at least GX_H * 128 doubles, see launch_gradx)
    __syncthreads();
    double *red = sm;   // [GX_H - 1][128], one dimension at a time
    for (int q = 0; q < GCH; ++q) {   // (uniform trip count: the barriers are met by every lane)
        if (d0 + q >= D) break;
        double mine = 0.0;
#pragma unroll
        for (int k = 0; k < GCH; ++k) mine = (k == q) ? acc[k] : mine;   // acc stays in registers: no dynamic index
        if (h > 0) red[(h - 1) * GP_TILE + r] = mine;
        __syncthreads();
        if (h == 0) {
            double v = mine;
#pragma unroll
            for (int k = 0; k < GX_H - 1; ++k) v += red[k * GP_TILE + r];
            partial[((long)blockIdx.y * Npad + gi) * GCH + q] = v;
        }
        __syncthreads();
    }
}

// out[i, d0 + q] = (sum over the chunks, ascending) / l_q for i < N: (x - x') / l^2 = scaled difference / l
__device__ __forceinline__ void gradx_sum_body(const double *partial, long N, long Npad, int nchunk, const KernParams &kp, int d0,
                                               double *out) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    const long i = e / GCH;
    const int q = (int)(e - i * GCH);
    if (i >= N || d0 + q >= kp.D) return;
    double s = 0.0;
    for (int k = 0; k < nchunk; ++k) s += partial[((long)k * Npad + i) * GCH + q];
    out[i * kp.D + d0 + q] = s / kp.ls[d0 + q];
}
__global__ __launch_bounds__(256) void gradx_sum_kernel(const double *partial, long N, long Npad, int nchunk, KernParams kp, int d0,
                                                        double *out) {
    gradx_sum_body(partial, N, Npad, nchunk, kp, d0, out);
}
__global__ __launch_bounds__(256) void gradx_sum_batch_kernel(const double *partial, long sP, long N, long Npad, int nchunk,
                                                              const KernParams *kpt, int d0, double *out, long so) {
    const long z = blockIdx.z;
    gradx_sum_body(partial + z * sP, N, Npad, nchunk, kpt[z], d0, out + z * so);
}

long gradx_partial_elems(long Npad) {
    const long nt = Npad / GP_TILE;
    return (nt + GX_CHUNK - 1) / GX_CHUNK * Npad * GCH;
}

// LDS of one workgroup of gradx_tile_kernel in bytes (all of it dynamic): the row and the column tile of the inputs and of alpha,
// and never less than the reduction's GX_H - 1 rows of 128 (held against the device's limit by gradx_lds_check, api_grad.hip)
size_t gradx_lds_bytes(int D, int P) {
    const size_t stage = ((size_t)2 * D * GP_TILE + (size_t)2 * P * GP_TILE) * sizeof(double);
    return std::max(stage, (size_t)GX_H * GP_TILE * sizeof(double));
}

// out (device, [N, D] row-major): dL/dX of every training row; partial: gradx_partial_elems(Npad) doubles of scratch
// nb > 1: the same passes for nb members, member z with inputs X + z sX, parameters kpt[z] (device), alpha + z sV, Ky^-1 at
// Wi + z sW, partials at partial + z sP and rows at out + z so; kp (the first member's, host) gives D and the family: the instance
// and the LDS size
void launch_gradx(hipStream_t s, const double *X, long N, long Npad, const KernParams &kp, const double *alpha, int P,
                  const double *Wi, long ldw, double *partial, double *out, int nb, const KernParams *kpt, long sX, long sV,
                  long sW, long sP, long so) {
    const int nt = (int)(Npad / GP_TILE);
    const int nchunk = (nt + GX_CHUNK - 1) / GX_CHUNK;
    const size_t shm = gradx_lds_bytes(kp.D, P);
    const int fp = GP_FAMILY_PAIR(kp.kernel);
    const dim3 grid((unsigned)nt, (unsigned)nchunk, (unsigned)nb);
    for (int d0 = 0; d0 < kp.D; d0 += GCH) {
        if (nb > 1) {
            if (fp)
                GP_LAUNCH((gradx_tile_kernel<1, 1>), grid, dim3(GX_THREADS), shm, s, X, sX, N, Npad, kp, kpt, d0, alpha, sV, Npad, P, Wi,
                          sW, ldw, partial, sP);
            else
                GP_LAUNCH((gradx_tile_kernel<0, 1>), grid, dim3(GX_THREADS), shm, s, X, sX, N, Npad, kp, kpt, d0, alpha, sV, Npad, P, Wi,
                          sW, ldw, partial, sP);
            GP_LAUNCH(gradx_sum_batch_kernel, dim3((unsigned)((N * GCH + 255) / 256), 1, (unsigned)nb), dim3(256), 0, s, partial, sP,
                      N, Npad, nchunk, kpt, d0, out, so);
            continue;
        }
        if (fp)
            GP_LAUNCH((gradx_tile_kernel<1, 0>), grid, dim3(GX_THREADS), shm, s, X, 0L, N, Npad, kp, nullptr, d0, alpha, 0L, Npad, P, Wi,
                      0L, ldw, partial, 0L);
        else
            GP_LAUNCH((gradx_tile_kernel<0, 0>), grid, dim3(GX_THREADS), shm, s, X, 0L, N, Npad, kp, nullptr, d0, alpha, 0L, Npad, P, Wi,
                      0L, ldw, partial, 0L);
        GP_LAUNCH(gradx_sum_kernel, dim3((unsigned)((N * GCH + 255) / 256)), dim3(256), 0, s, partial, N, Npad, nchunk, kp, d0, out);
    }
}

// ---- Kumaraswamy warp of a candidate table, in place ------------------------------------------------------------------
// w_q(x) = 1 - (1 - u^a_q)^b_q, u = (x - xmin_q) / (xmax_q - xmin_q) where warp[q] is set; the value itself where not.
// Two elements (16 bytes) per lane; the table's base is 16-byte aligned and e0 (the first element's index in the whole
// table, for the column) even, so a pair never straddles the launch's range except in its last, odd element.
struct KumarParams {
    int D;
    unsigned char warp[GP_MAX_D];
    double a[GP_MAX_D], b[GP_MAX_D], xmin[GP_MAX_D], xmax[GP_MAX_D];
};
__device__ __forceinline__ double kumar_one(const KumarParams &kw, int q, double x) {
    if (!kw.warp[q]) return x;
    const double u = (x - kw.xmin[q]) / (kw.xmax[q] - kw.xmin[q]);
    return 1.0 - pow(1.0 - pow(u, kw.a[q]), kw.b[q]);
}
__global__ __launch_bounds__(256) void kumar_warp_kernel(double *T, long e0, long n, KumarParams kw) {
    const long k = ((long)blockIdx.x * 256 + threadIdx.x) * 2;
    if (k >= n) return;
    const int q0 = (int)((e0 + k) % kw.D);
    if (k + 1 < n) {
        double2_t v = *(const double2_t *)(T + k);
        const int q1 = (q0 + 1 == kw.D) ? 0 : q0 + 1;
        v[0] = kumar_one(kw, q0, v[0]);
        v[1] = kumar_one(kw, q1, v[1]);
        *(double2_t *)(T + k) = v;
    } else {
        T[k] = kumar_one(kw, q0, T[k]);
    }
}
// rows [m0, m0 + mc) of the resident [M, D] table Xs
void launch_kumar_warp(hipStream_t s, double *Xs, long m0, long mc, int D, const int *warp, const double *a, const double *b,
                       const double *xmin, const double *xmax) {
    KumarParams kw;
    memset(&kw, 0, sizeof(kw));
    kw.D = D;
    for (int q = 0; q < D; ++q) {
        kw.warp[q] = warp[q] ? 1 : 0;
        kw.a[q] = a[q];
        kw.b[q] = b[q];
        kw.xmin[q] = xmin[q];
        kw.xmax[q] = xmax[q];
    }
    const long e0 = m0 * D, n = mc * D;
    GP_LAUNCH(kumar_warp_kernel, dim3((unsigned)((n / 2 + 1 + 255) / 256)), dim3(256), 0, s, Xs + e0, e0, n, kw);
}
