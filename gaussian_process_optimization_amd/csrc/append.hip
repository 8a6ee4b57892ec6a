// Growing a factor by k <= 128 rows that lie inside ONE diagonal tile (gp_append, api_append.hip): with T = L11^-1 K(X, Xnew),
//   S = K(Xnew, Xnew) + d I - T^T T,   L22 = chol(S),   L21 = T^T,   Li21 = -L22^-1 (L21 Li11),   Li22 = L22^-1.
// Everything here streams: the only O(N^2) work is one read of the lower triangle of L^-1 per eight new rows and direction
// (row dots for T, column sums for L21 Li11); the k x k factorisation itself is the diagonal-tile kernel of potrf.hip on a
// scratch tile padded with the identity.  Every sum has one writer and a fixed order: the same input gives the same bits.
// The border is computed into scratch; the factor's rows are written by append_commit_rows_kernel only, after the host has
// seen the pivots.
#include "gphip_internal.h"

#define AP_V 8            // vectors (new rows) per pass over the matrix
#define AP_RPW 4          // row dots: rows per wave
#define AP_COLCH 1024     // column sums: rows per workgroup

template <bool NT>
__device__ __forceinline__ double2_t ap_load2(const double *p) {
    if (NT) return __builtin_nontemporal_load((const double2_t *)p);
    return *(const double2_t *)p;
}
__device__ __forceinline__ double ap_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}

// O[c ldo + i] = sum_{j <= i} Mat[i ld + j] V[c ldv + j]   for i < n, c < kc <= AP_V.  Mat: lower triangular, row-major, exact zeros
// above the diagonal, ncols (even) allocated columns; V zero or finite up to ncols.  A wave takes AP_RPW rows, lane l the column
// pairs 2 l (+ 128) of each 256-column chunk, with the vectors' matching elements in registers for all of its rows.
template <bool NT>
__global__ __launch_bounds__(256) void append_rowdot_kernel(const double *Mat, long ld, long n, long ncols, const double *V, long ldv,
                                                            int kc, double *O, long ldo) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const long rbase = ((long)blockIdx.x * 4 + wave) * AP_RPW;
    if (rbase >= n) return;
    const long ilast = min(rbase + AP_RPW - 1, n - 1);
    const long jend = min(ncols, (ilast + 2) & ~1L);   // the rows' entries beyond are zeros
    double acc[AP_RPW][AP_V];
#pragma unroll
    for (int r = 0; r < AP_RPW; ++r)
#pragma unroll
        for (int c = 0; c < AP_V; ++c) acc[r][c] = 0.0;
    const double2_t zero2 = {0.0, 0.0};
    for (long j0 = 0; j0 < jend; j0 += 256) {
        const long ja = j0 + 2 * lane, jb = ja + 128;
        double2_t va[AP_V], vb[AP_V];
#pragma unroll
        for (int c = 0; c < AP_V; ++c) {
            va[c] = (c < kc && ja < jend) ? *(const double2_t *)(V + (long)c * ldv + ja) : zero2;
            vb[c] = (c < kc && jb < jend) ? *(const double2_t *)(V + (long)c * ldv + jb) : zero2;
        }
#pragma unroll
        for (int r = 0; r < AP_RPW; ++r) {
            const long row = rbase + r;
            if (row >= n) break;
            const double *mp = Mat + row * ld;
            const double2_t xa = ja < jend ? ap_load2<NT>(mp + ja) : zero2;
            const double2_t xb = jb < jend ? ap_load2<NT>(mp + jb) : zero2;
#pragma unroll
            for (int c = 0; c < AP_V; ++c) {
                double s = fma(xa[0], va[c][0], xa[1] * va[c][1]);
                s = fma(xb[0], vb[c][0], fma(xb[1], vb[c][1], s));
                acc[r][c] += s;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < AP_RPW; ++r) {
        const long row = rbase + r;
        if (row >= n) break;
#pragma unroll
        for (int c = 0; c < AP_V; ++c) {
            const double s = ap_wave_sum(acc[r][c]);
            if (lane == 0 && c < kc) O[(long)c * ldo + row] = s;
        }
    }
}

void launch_append_rowdot(hipStream_t s, const double *Mat, long ld, long n, long ncols, const double *V, long ldv, int kc, double *O,
                          long ldo, int nt_loads) {
    if (n <= 0 || kc <= 0) return;
    const dim3 grid((unsigned)((n + 4 * AP_RPW - 1) / (4 * AP_RPW)));
    if (nt_loads) GP_LAUNCH(append_rowdot_kernel<true>, grid, dim3(256), 0, s, Mat, ld, n, ncols, V, ldv, kc, O, ldo);
    else GP_LAUNCH(append_rowdot_kernel<false>, grid, dim3(256), 0, s, Mat, ld, n, ncols, V, ldv, kc, O, ldo);
}

// Column sums  R[c][j] = sum_{i = j}^{n - 1} V[c ldv + i] Mat[i ld + j]  of the same matrix, as partials: workgroup (strip, q) owns
// the 128 columns of its strip and walks down the rows [max(128 strip, q AP_COLCH), min(n, (q + 1) AP_COLCH)) -- a strip starts at
// its diagonal, the zeros above it are never read -- one row of the strip per wave instruction (lane l: columns 2 l, 2 l + 1), the
// four waves taking every fourth row.  part[(q AP_V + c) ldp + j]; a (strip, q) with no rows writes nothing and is never read
// (append_colreduce_kernel sums q from the strip's first chunk on).
template <bool NT>
__global__ __launch_bounds__(256) void append_colpass_kernel(const double *Mat, long ld, long n, const double *V, long ldv, int kc,
                                                             double *part, long ldp) {
    __shared__ __attribute__((aligned(16))) double sh[4][AP_V][GP_TILE];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const long c0 = (long)blockIdx.x * GP_TILE;
    const long q = blockIdx.y;
    const long rlo = max(c0, q * AP_COLCH), rhi = min(n, (q + 1) * AP_COLCH);
    if (rlo >= rhi) return;
    double2_t acc[AP_V];
#pragma unroll
    for (int c = 0; c < AP_V; ++c) acc[c] = (double2_t){0.0, 0.0};
    const double *mp = Mat + c0 + 2 * lane;
    long i = rlo + wave;
    for (; i + 12 < rhi; i += 16) {   // four rows of this wave in flight
        double2_t x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = ap_load2<NT>(mp + (i + 4 * u) * ld);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int c = 0; c < AP_V; ++c) {
                const double v = c < kc ? V[(long)c * ldv + i + 4 * u] : 0.0;
                acc[c][0] = fma(v, x[u][0], acc[c][0]);
                acc[c][1] = fma(v, x[u][1], acc[c][1]);
            }
    }
    for (; i < rhi; i += 4) {
        const double2_t x = ap_load2<NT>(mp + i * ld);
#pragma unroll
        for (int c = 0; c < AP_V; ++c) {
            const double v = c < kc ? V[(long)c * ldv + i] : 0.0;
            acc[c][0] = fma(v, x[0], acc[c][0]);
            acc[c][1] = fma(v, x[1], acc[c][1]);
        }
    }
#pragma unroll
    for (int c = 0; c < AP_V; ++c) *(double2_t *)&sh[wave][c][2 * lane] = acc[c];
    __syncthreads();
    for (int e = threadIdx.x; e < AP_V * GP_TILE; e += 256) {
        const int c = e / GP_TILE, j = e % GP_TILE;
        if (c < kc) part[(q * AP_V + c) * ldp + c0 + j] = ((sh[0][c][j] + sh[1][c][j]) + sh[2][c][j]) + sh[3][c][j];
    }
}
// R[c ldr + j] = the partials of column j summed in chunk order for j < n, 0 for n <= j < ncols
__global__ __launch_bounds__(256) void append_colreduce_kernel(const double *part, long ldp, long n, long ncols, int nq, double *R, long ldr) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y;
    if (j >= ncols) return;
    double s = 0.0;
    if (j < n)
        for (long q = (j / GP_TILE * GP_TILE) / AP_COLCH; q < nq; ++q) s += part[(q * AP_V + c) * ldp + j];
    R[(long)c * ldr + j] = s;
}

int append_col_chunks(long n) { return (int)((n + AP_COLCH - 1) / AP_COLCH); }
// R[c ldr + j], c < kc <= AP_V, j < ncols (zero from n on) through part: append_col_chunks(n) AP_V ldp doubles, ldp >= round_up(n, 128)
void launch_append_colsum(hipStream_t s, const double *Mat, long ld, long n, long ncols, const double *V, long ldv, int kc, double *part,
                          long ldp, double *R, long ldr, int nt_loads) {
    if (ncols <= 0 || kc <= 0) return;
    const int nq = append_col_chunks(n);
    if (n > 0) {
        const dim3 grid((unsigned)((n + GP_TILE - 1) / GP_TILE), (unsigned)nq);
        if (nt_loads) GP_LAUNCH(append_colpass_kernel<true>, grid, dim3(256), 0, s, Mat, ld, n, V, ldv, kc, part, ldp);
        else GP_LAUNCH(append_colpass_kernel<false>, grid, dim3(256), 0, s, Mat, ld, n, V, ldv, kc, part, ldp);
    }
    GP_LAUNCH(append_colreduce_kernel, dim3((unsigned)((ncols + 255) / 256), (unsigned)kc), dim3(256), 0, s, part, ldp, n, ncols, nq, R, ldr);
}

// ---- the border's k x k Gram  G = T T^T  (T: k rows of n entries) as partials over 1024-column chunks: workgroup (chunk, a) holds
// row a's chunk in registers and dots it with every row b <= a, one wave per b.  gpart[(chunk k + a) k + b]
__global__ __launch_bounds__(256) void append_gram_kernel(const double *T, long ldt, long n, int k, double *gpart) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int a = blockIdx.y;
    const long j0 = (long)blockIdx.x * 1024;
    const double2_t zero2 = {0.0, 0.0};
    double2_t ta[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const long j = j0 + 2 * lane + 128 * u;   // (n may be odd: the pair's second entry is masked)
        ta[u] = zero2;
        if (j < n) ta[u][0] = T[(long)a * ldt + j];
        if (j + 1 < n) ta[u][1] = T[(long)a * ldt + j + 1];
    }
    for (int b = wave; b <= a; b += 4) {
        double s = 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const long j = j0 + 2 * lane + 128 * u;
            const double t0 = j < n ? T[(long)b * ldt + j] : 0.0, t1 = j + 1 < n ? T[(long)b * ldt + j + 1] : 0.0;
            s = fma(ta[u][0], t0, fma(ta[u][1], t1, s));
        }
        s = ap_wave_sum(s);
        if (lane == 0) gpart[((long)blockIdx.x * k + a) * k + b] = s;
    }
}
// The scratch tile S (128 x 128, symmetric, identity beyond k) the diagonal-tile kernel factors: S = Knn + d I - G, its diagonal by
// the rule of kbuild.hip -- exactly the variance (Euclidean) or the Gower product already in Knn, plus diag_add, then the jitter.
// flag[0] = 1 where an entry is not finite.
__global__ __launch_bounds__(256) void append_schur_kernel(const double *gpart, int nchunks, int k, const double *Knn, double variance,
                                                           int gower, double diag_add, double jitter, double *S, int *flag) {
    for (int e = threadIdx.x; e < GP_TILE * GP_TILE; e += 256) {
        const int a = e / GP_TILE, b = e % GP_TILE;
        if (a >= k || b >= k) {
            S[e] = a == b ? 1.0 : 0.0;
            continue;
        }
        if (b > a) continue;
        double gsum = 0.0;
        for (int q = 0; q < nchunks; ++q) gsum += gpart[((long)q * k + a) * k + b];
        double v = Knn[a * GP_TILE + b];
        if (a == b) v = ((gower ? v : variance) + diag_add) + jitter;
        v -= gsum;
        if (!isfinite(v)) flag[0] = 1;
        S[a * GP_TILE + b] = v;
        S[b * GP_TILE + a] = v;
    }
}
void launch_append_schur(hipStream_t s, const double *T, long ldt, long n, int k, double *gpart, const double *Knn, double variance,
                         int gower, double diag_add, double jitter, double *S, int *flag) {
    const int nchunks = (int)((n + 1023) / 1024);
    if (nchunks > 0) GP_LAUNCH(append_gram_kernel, dim3((unsigned)nchunks, (unsigned)k), dim3(256), 0, s, T, ldt, n, k, gpart);
    GP_LAUNCH(append_schur_kernel, dim3(1), dim3(256), 0, s, gpart, nchunks, k, Knn, variance, gower, diag_add, jitter, S, flag);
}
long append_gram_elems(long n, int k) { return ((n + 1023) / 1024) * (long)k * k; }

// O[a ldo + j] = -sum_{b <= a} Linv[a 128 + b] R[b ldr + j]   for a < k, j < ncols  (Li21 = -L22^-1 R)
__global__ __launch_bounds__(256) void append_negmul_kernel(const double *Linv, const double *R, long ldr, int k, long ncols, double *O,
                                                            long ldo) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    const int a = blockIdx.y;
    if (j >= ncols) return;
    double s = 0.0;
    for (int b = 0; b <= a; ++b) s = fma(Linv[a * GP_TILE + b], R[(long)b * ldr + j], s);
    O[(long)a * ldo + j] = -s;
}
void launch_append_negmul(hipStream_t s, const double *Linv, const double *R, long ldr, int k, long ncols, double *O, long ldo) {
    if (ncols <= 0 || k <= 0) return;
    GP_LAUNCH(append_negmul_kernel, dim3((unsigned)((ncols + 255) / 256), (unsigned)k), dim3(256), 0, s, Linv, R, ldr, k, ncols, O, ldo);
}

// Rows row0 .. row0 + k - 1 of dst (ld, ncols columns):  [ src21 (columns < c0) | lower triangle of tile22 (columns c0 .. c0 + k) | 0 ]
__global__ __launch_bounds__(256) void append_commit_rows_kernel(double *dst, long ld, long ncols, long row0, int k, long c0,
                                                                 const double *src21, long ld21, const double *tile22) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    const int a = blockIdx.y;
    if (j >= ncols) return;
    double v = 0.0;
    if (j < c0) v = src21[(long)a * ld21 + j];
    else if (j - c0 <= a) v = tile22[a * GP_TILE + (j - c0)];
    dst[(row0 + a) * ld + j] = v;
}
void launch_append_commit_rows(hipStream_t s, double *dst, long ld, long ncols, long row0, int k, long c0, const double *src21, long ld21,
                               const double *tile22) {
    if (k <= 0) return;
    GP_LAUNCH(append_commit_rows_kernel, dim3((unsigned)((ncols + 255) / 256), (unsigned)k), dim3(256), 0, s, dst, ld, ncols, row0, k, c0,
              src21, ld21, tile22);
}

// Rows r0 .. r1 - 1 of dst (ld, ncols columns) as rows of the identity: the padding of a tile
__global__ __launch_bounds__(256) void append_identity_rows_kernel(double *dst, long ld, long ncols, long r0) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    const long r = r0 + blockIdx.y;
    if (j < ncols) dst[r * ld + j] = j == r ? 1.0 : 0.0;
}
void launch_append_identity_rows(hipStream_t s, double *dst, long ld, long ncols, long r0, long r1) {
    if (r1 <= r0) return;
    GP_LAUNCH(append_identity_rows_kernel, dim3((unsigned)((ncols + 255) / 256), (unsigned)(r1 - r0)), dim3(256), 0, s, dst, ld, ncols, r0);
}

// O[p ldo + i] = Y[i P + p] for i < N, 0 for N <= i < ncols: the targets as rows (the right-hand sides of z = L^-1 Y)
__global__ __launch_bounds__(256) void append_yrows_kernel(const double *Y, long N, int P, long ncols, double *O, long ldo) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int p = blockIdx.y;
    if (i < ncols) O[(long)p * ldo + i] = i < N ? Y[i * P + p] : 0.0;
}
void launch_append_yrows(hipStream_t s, const double *Y, long N, int P, long ncols, double *O, long ldo) {
    GP_LAUNCH(append_yrows_kernel, dim3((unsigned)((ncols + 255) / 256), (unsigned)P), dim3(256), 0, s, Y, N, P, ncols, O, ldo);
}
