// The cost surface of cost-aware EI / MPI (GPyOpt/core/task/cost.py: cost = exp(m_c), m_c the posterior mean of a GP over the
// logarithm of the evaluation times) and the quotient it puts under the scores (acquisitions/base.py:47-50).
//
//   logc(x)      = shift + scale sum_j alpha_j k(x, Xc_j)
//   dlogc(x)/dx_d = scale / l_d sum_j alpha_j g(r_j) (x_d - Xc_jd) / l_d,      g = dK_dr / r  (gphip_internal.h)
//
// over a snapshot of the cost GP: Xcs = Xc / lengthscale [Nc, ld] (scaled once, on the host, when the surface is set), alpha [Nc],
// the kernel's parameters and the normaliser (shift, scale).  A posterior mean needs no factor.
//
// ONE summation order per location, whatever the launch geometry: the Nc terms are cut into chunks of COST_CB consecutive rows; a
// chunk's terms are accumulated from 0 in row order by fma (cost_chunk, the only place the terms are formed), and the chunks'
// partial sums are added to the running total in chunk order.  The table kernel (one candidate per thread, tiles of the surface
// staged through LDS and shared by the workgroup's candidates) runs that order in one thread; the few-rows kernel (one workgroup
// per location) deals the chunks over its threads and adds their partials in the same order afterwards; a table of few rows and
// values only is cut along the surface as well (slices of whole tiles as a second grid dimension, the chunks' partial sums written
// out and added in order by cost_table_combine_kernel), so that 10^4 candidates reach every compute unit.  Same operations on
// the same operands in the same order: the bits of a location do not depend on its company.
//
// Plain fp64 FMA, no MFMA: per pair D subtractions and D fma for r^2, one sqrt and one exp (Matern) and a dozen multiply-adds for
// k and g, 1 + D fma for the sums -- the pass is bound by exp / sqrt and the vector ALU, not by the matrix pipe.
#include "gphip_internal.h"

#define COST_CB 32        // terms per chunk of the summation order
#define COST_DCH 8        // gradient dimensions per pass (D <= 8: one pass, the location's coordinates in registers)
#define COST_TJ 128       // rows of the surface per LDS tile of the table kernel (a whole number of chunks) ...
#define COST_TJ_WIDE 32   // ... and where D > 8: the tile and the candidates' coordinates share 64 KB of LDS up to GP_MAX_D
#define COST_ROWS_T 256   // threads (= chunks per round) of the few-rows kernel
static_assert(COST_TJ % COST_CB == 0 && COST_TJ_WIDE % COST_CB == 0, "tiles hold whole chunks");

// the location's scaled coordinates: in registers, zero beyond D (D <= COST_DCH; the surface's rows are padded alike) ...
struct CostXsReg {
    double x[COST_DCH];
    __device__ __forceinline__ double operator()(int d) const { return x[d]; }
};
// ... or in LDS, `stride` doubles between two dimensions (the table: one column per thread; the few rows: stride 1)
struct CostXsLds {
    const double *p;
    int stride;
    __device__ __forceinline__ double operator()(int d) const { return p[(long)d * stride]; }
};

// The partial sums of ONE chunk: rows [0, n) at xc (scaled, ld doubles apart) with weights al; v the value's, gd[q] that of
// gradient dimension d0 + q.  REG: D <= COST_DCH, every loop runs over the COST_DCH padded dimensions (the zeros add exactly 0).
template <bool REG, bool GRAD, class XS>
__device__ __forceinline__ void cost_chunk(int kernel, double variance, const double *xc, int ld, const double *al, int n, int D,
                                           int d0, const XS &xs, double &v, double *gd) {
    v = 0.0;
#pragma unroll
    for (int q = 0; q < COST_DCH; ++q) gd[q] = 0.0;
    for (int j = 0; j < n; ++j) {
        const double *row = xc + (long)j * ld;
        double s = 0.0;
        if (REG) {
#pragma unroll
            for (int d = 0; d < COST_DCH; ++d) {
                const double df = xs(d) - row[d];
                s = fma(df, df, s);
            }
        } else {
            for (int d = 0; d < D; ++d) {
                const double df = xs(d) - row[d];
                s = fma(df, df, s);
            }
        }
        double k, g;
        gp_k_and_g(kernel, variance, s, k, g);
        const double a = al[j];
        v = fma(k, a, v);
        if (GRAD) {
            const double t = g * a;
#pragma unroll
            for (int q = 0; q < COST_DCH; ++q) {
                const int d = d0 + q;
                if (REG || d < D) gd[q] = fma(t, xs(d) - row[d], gd[q]);
            }
        }
    }
}
// what the totals become
__device__ __forceinline__ double cost_logc(double tot, double shift, double scale) { return fma(scale, tot, shift); }
__device__ __forceinline__ double cost_dlogc(double gtot, double scale, double l) { return (scale * gtot) / l; }

// ---- the table: one candidate per thread ----------------------------------------------------------------------------------------
// LDS: tile [TJ][ld], at [TJ], and without REG the candidates' scaled coordinates [D][blockDim.x]; TJ = COST_TJ (REG) / COST_TJ_WIDE.
// part null: the whole surface, logc / dlogc written.  part given (values only): slice blockIdx.y of slice_tiles tiles, the partial
// sum of chunk c of candidate i to part[c M + i] and nothing else.
template <bool REG, bool GRAD>
__global__ __launch_bounds__(256) void cost_table_kernel(const double *Xs, long M, const double *Xcs, int ld, const double *alpha, long Nc,
                                                         KernParams kp, double shift, double scale, double *logc, double *dlogc,
                                                         double *part, int slice_tiles) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    constexpr int TJ = REG ? COST_TJ : COST_TJ_WIDE;
    double *tile = sm, *at = sm + (long)TJ * ld, *xl = at + TJ;
    const int tid = threadIdx.x, nthr = blockDim.x, D = kp.D;
    const long i = (long)blockIdx.x * nthr + tid;
    const long ic = i < M ? i : M - 1;   // (the spare threads of the last workgroup stage and synchronise with the rest)
    CostXsReg xr;
    if (REG) {
#pragma unroll
        for (int d = 0; d < COST_DCH; ++d) xr.x[d] = d < D ? Xs[ic * D + d] / kp_div(kp, d) : 0.0;
    } else {
        for (int d = 0; d < D; ++d) xl[(long)d * nthr + tid] = Xs[ic * D + d] / kp_div(kp, d);
    }
    const CostXsLds xq{xl + tid, nthr};
    const int npass = (REG || !GRAD) ? 1 : (D + COST_DCH - 1) / COST_DCH;
    for (int pass = 0; pass < npass; ++pass) {
        const int d0 = pass * COST_DCH;
        double tot = 0.0, gtot[COST_DCH];
#pragma unroll
        for (int q = 0; q < COST_DCH; ++q) gtot[q] = 0.0;
        const long jb = part ? (long)blockIdx.y * slice_tiles * TJ : 0;
        const long je = part ? (jb + (long)slice_tiles * TJ < Nc ? jb + (long)slice_tiles * TJ : Nc) : Nc;
        for (long j0 = jb; j0 < je; j0 += TJ) {
            const int nrow = (int)(je - j0 < TJ ? je - j0 : TJ);
            __syncthreads();
            for (int idx = tid; idx < nrow * ld; idx += nthr) tile[idx] = Xcs[j0 * ld + idx];
            for (int idx = tid; idx < nrow; idx += nthr) at[idx] = alpha[j0 + idx];
            __syncthreads();
            for (int c0 = 0; c0 < nrow; c0 += COST_CB) {
                const int n = nrow - c0 < COST_CB ? nrow - c0 : COST_CB;
                double v, gd[COST_DCH];
                if (REG) cost_chunk<true, GRAD>(kp.kernel, kp.variance, tile + (long)c0 * ld, ld, at + c0, n, D, d0, xr, v, gd);
                else cost_chunk<false, GRAD>(kp.kernel, kp.variance, tile + (long)c0 * ld, ld, at + c0, n, D, d0, xq, v, gd);
                if (!GRAD && part) {
                    if (i < M) part[(j0 + c0) / COST_CB * M + i] = v;
                    continue;
                }
                tot = tot + v;
                if (GRAD) {
#pragma unroll
                    for (int q = 0; q < COST_DCH; ++q) gtot[q] = gtot[q] + gd[q];
                }
            }
        }
        if (i < M && !(!GRAD && part)) {
            if (pass == 0) logc[i] = cost_logc(tot, shift, scale);
            if (GRAD) {
#pragma unroll
                for (int q = 0; q < COST_DCH; ++q)
                    if (d0 + q < D) dlogc[i * D + d0 + q] = cost_dlogc(gtot[q], scale, kp_div(kp, d0 + q));
            }
        }
    }
}

// the chunks' partial sums of the sliced launch, added in chunk order
__global__ void cost_table_combine_kernel(const double *part, long M, long nchunk, double shift, double scale, double *logc) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    double tot = 0.0;
    for (long c = 0; c < nchunk; ++c) tot = tot + part[c * M + i];
    logc[i] = cost_logc(tot, shift, scale);
}

size_t cost_table_lds_bytes(int D, int ld, int threads) {
    const size_t tj = D > COST_DCH ? COST_TJ_WIDE : COST_TJ;
    return sizeof(double) * (tj * ld + tj + (D > COST_DCH ? (size_t)D * threads : 0));
}
// threads per workgroup: 256 with the coordinates in registers; 64 where they live in LDS (D > 8: 64 D + 32 (D + 1) doubles, 49 KB
// at GP_MAX_D).  Tables of few rows take 64 either way, to reach more compute units (the bits do not depend on it).
int cost_table_threads(long M, int D) { return (D > COST_DCH || M <= 64 * 256) ? 64 : 256; }

// Slices of a values-only launch: enough to bring the grid to COST_SPLIT_WGS workgroups (four per compute unit), none where the
// table fills the device by itself, the surface has fewer than COST_SPLIT_MIN_CHUNKS chunks, or the partial sums would exceed
// COST_SPLIT_MAX_PART doubles.  Returns the tiles per slice (0: no slices) and the slices.
#define COST_SPLIT_WGS 1024
#define COST_SPLIT_MIN_CHUNKS 8
#define COST_SPLIT_MAX_PART (16L << 20)
static int cost_table_slices(long M, long Nc, int D, int *slices) {
    const long tj = D > COST_DCH ? COST_TJ_WIDE : COST_TJ, ntile = (Nc + tj - 1) / tj, nchunk = (Nc + COST_CB - 1) / COST_CB;
    const long wgs = (M + cost_table_threads(M, D) - 1) / cost_table_threads(M, D);
    const long want = std::min<long>((COST_SPLIT_WGS + wgs - 1) / wgs, ntile);
    if (want < 2 || nchunk < COST_SPLIT_MIN_CHUNKS || M * nchunk > COST_SPLIT_MAX_PART) return 0;
    const long per = (ntile + want - 1) / want;
    *slices = (int)((ntile + per - 1) / per);
    return (int)per;
}
size_t cost_table_part_elems(long M, long Nc, int D) {
    int slices = 0;
    return cost_table_slices(M, Nc, D, &slices) ? (size_t)M * (size_t)((Nc + COST_CB - 1) / COST_CB) : 0;
}

void launch_cost_table(hipStream_t s, const double *Xs, long M, const double *Xcs, int ld, const double *alpha, long Nc,
                       const KernParams &kp, double shift, double scale, double *logc, double *dlogc, double *part) {
    if (M <= 0) return;
    const int thr = cost_table_threads(M, kp.D);
    const size_t lds = cost_table_lds_bytes(kp.D, ld, thr);
    int slices = 1;
    const int per = (!dlogc && part) ? cost_table_slices(M, Nc, kp.D, &slices) : 0;
    if (!per) {
        part = nullptr;
        slices = 1;
    }
    const dim3 grid((unsigned)((M + thr - 1) / thr), (unsigned)slices), block(thr);
    if (kp.D <= COST_DCH) {
        if (dlogc) GP_LAUNCH((cost_table_kernel<true, true>), grid, block, lds, s, Xs, M, Xcs, ld, alpha, Nc, kp, shift, scale, logc, dlogc, part, per);
        else GP_LAUNCH((cost_table_kernel<true, false>), grid, block, lds, s, Xs, M, Xcs, ld, alpha, Nc, kp, shift, scale, logc, dlogc, part, per);
    } else {
        if (dlogc) GP_LAUNCH((cost_table_kernel<false, true>), grid, block, lds, s, Xs, M, Xcs, ld, alpha, Nc, kp, shift, scale, logc, dlogc, part, per);
        else GP_LAUNCH((cost_table_kernel<false, false>), grid, block, lds, s, Xs, M, Xcs, ld, alpha, Nc, kp, shift, scale, logc, dlogc, part, per);
    }
    if (part)
        GP_LAUNCH(cost_table_combine_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, part, M, (Nc + COST_CB - 1) / COST_CB, shift, scale, logc);
}

// ---- a few rows: one workgroup per location, the chunks dealt over its threads --------------------------------------------------
// blk null: logc [M] / dlogc [M, D] (null: values only) are written.  blk given: the quotient is applied in place to the negated
// score blk[2 MV + m] and, with GRAD, to its gradient blk[3 MV + 2 MV D + m D + d] of the rows layout (gphip_internal.h):
//   dneg <- (dneg - neg_old dlogc) / c ,  neg <- neg / c ,  c = exp(logc)
template <bool REG, bool GRAD>
__global__ __launch_bounds__(COST_ROWS_T) void cost_rows_kernel(RowsX rx, const double *Xcs, int ld, const double *alpha, long Nc,
                                                                KernParams kp, double shift, double scale, double *logc, double *dlogc,
                                                                double *blk, int MV) {
    __shared__ double part[COST_ROWS_T][COST_DCH + 1];
    __shared__ double xl[GP_MAX_D];
    __shared__ double head[2];   // logc of the location, the score as it came
    const int tid = threadIdx.x, D = kp.D, m = blockIdx.x;
    CostXsReg xr;
    if (REG) {
#pragma unroll
        for (int d = 0; d < COST_DCH; ++d) xr.x[d] = d < D ? rx.xs[m * D + d] / kp_div(kp, d) : 0.0;
    } else {
        for (int d = tid; d < D; d += COST_ROWS_T) xl[d] = rx.xs[m * D + d] / kp_div(kp, d);
    }
    if (blk && tid == 0) head[1] = blk[2 * MV + m];
    __syncthreads();
    const CostXsLds xq{xl, 1};
    const long nchunk = (Nc + COST_CB - 1) / COST_CB;
    const int npass = (REG || !GRAD) ? 1 : (D + COST_DCH - 1) / COST_DCH;
    for (int pass = 0; pass < npass; ++pass) {
        const int d0 = pass * COST_DCH;
        double tot = 0.0;   // thread 0: the value's total; thread 1 + q: that of gradient dimension d0 + q
        for (long cb = 0; cb < nchunk; cb += COST_ROWS_T) {
            const long c = cb + tid;
            if (c < nchunk) {
                const long j0 = c * COST_CB;
                const int n = (int)(Nc - j0 < COST_CB ? Nc - j0 : COST_CB);
                double v, gd[COST_DCH];
                if (REG) cost_chunk<true, GRAD>(kp.kernel, kp.variance, Xcs + j0 * ld, ld, alpha + j0, n, D, d0, xr, v, gd);
                else cost_chunk<false, GRAD>(kp.kernel, kp.variance, Xcs + j0 * ld, ld, alpha + j0, n, D, d0, xq, v, gd);
                part[tid][0] = v;
#pragma unroll
                for (int q = 0; q < COST_DCH; ++q) part[tid][1 + q] = gd[q];
            }
            __syncthreads();
            if (tid <= (GRAD ? COST_DCH : 0)) {
                const int cnt = (int)(nchunk - cb < COST_ROWS_T ? nchunk - cb : COST_ROWS_T);
                for (int t = 0; t < cnt; ++t) tot = tot + part[t][tid];
            }
            __syncthreads();
        }
        if (tid == 0 && pass == 0) head[0] = cost_logc(tot, shift, scale);
        __syncthreads();
        if (GRAD && tid >= 1 && tid <= COST_DCH && d0 + tid - 1 < D) {
            const int d = d0 + tid - 1;
            const double dl = cost_dlogc(tot, scale, kp_div(kp, d));
            if (blk) {
                double *gp = blk + 3 * MV + 2L * MV * D + (long)m * D + d;
                *gp = (*gp - head[1] * dl) / exp(head[0]);
            } else {
                dlogc[(long)m * D + d] = dl;
            }
        }
    }
    if (tid == 0) {
        if (blk) blk[2 * MV + m] = head[1] / exp(head[0]);
        else logc[m] = head[0];
    }
}

void launch_cost_rows(hipStream_t s, const RowsX &rx, const double *Xcs, int ld, const double *alpha, long Nc, const KernParams &kp,
                      double shift, double scale, int grad, double *logc, double *dlogc, double *blk, int MV) {
    const dim3 grid((unsigned)rx.M), block(COST_ROWS_T);
    if (kp.D <= COST_DCH) {
        if (grad) GP_LAUNCH((cost_rows_kernel<true, true>), grid, block, 0, s, rx, Xcs, ld, alpha, Nc, kp, shift, scale, logc, dlogc, blk, MV);
        else GP_LAUNCH((cost_rows_kernel<true, false>), grid, block, 0, s, rx, Xcs, ld, alpha, Nc, kp, shift, scale, logc, dlogc, blk, MV);
    } else {
        if (grad) GP_LAUNCH((cost_rows_kernel<false, true>), grid, block, 0, s, rx, Xcs, ld, alpha, Nc, kp, shift, scale, logc, dlogc, blk, MV);
        else GP_LAUNCH((cost_rows_kernel<false, false>), grid, block, 0, s, rx, Xcs, ld, alpha, Nc, kp, shift, scale, logc, dlogc, blk, MV);
    }
}

// ---- the quotient over a table, element-wise, in place --------------------------------------------------------------------------
// neg [M] negated scores, dneg [M, D] their gradients (null: values only), dlogc [M, D]
__global__ void cost_apply_kernel(const double *logc, const double *dlogc, long M, int D, double *neg, double *dneg) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const double c = exp(logc[i]), old = neg[i];
    if (dneg)
        for (int d = 0; d < D; ++d) dneg[i * D + d] = (dneg[i * D + d] - old * dlogc[i * D + d]) / c;
    neg[i] = old / c;
}
void launch_cost_apply(hipStream_t s, const double *logc, const double *dlogc, long M, int D, double *neg, double *dneg) {
    if (M <= 0) return;
    GP_LAUNCH(cost_apply_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, logc, dlogc, M, D, neg, dneg);
}
