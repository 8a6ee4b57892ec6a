// The discrete knowledge gradient (Frazier, Powell & Dayanik 2009; Scott, Frazier & Powell 2011): the expected decrease of the minimum
// of the posterior mean over the A resident discretisation points and the location itself after one more observation there,
//     KG(x) = -E_Z[ min_i (a~_i + b_i Z) ],   Z ~ N(0, 1),   i = 0 .. A  (include/gphip.h has the definition of the A + 1 lines).
// The expectation is the lower envelope of the lines in closed form.  INTERVAL form: thread i intersects the half-lines
// (b_i - b_j) z <= a~_j - a~_i over all j -- no sort, no data-dependent control flow beyond the tie rule -- and owns [lo_i, hi_i];
// the breakpoint of a pair is the same bits seen from either side, so the intervals tile the axis.  One device function
// (kg_envelope) serves the table kernel and the rows kernel.  Always true fp64; every sum has a fixed order, no atomics but the rows
// path's arrival counter: a location's value and gradient depend on nothing but its own lines.
//
// Kernels:
//   kg_score_kernel   table: one workgroup per candidate over its row of C = K(Xs, X_A) - (K(Xs, X) L^-T) V_A^T
//   kg_rows_kernel    behind the fused rows path's forward pass (es_rows_kernel's geometry): the shares of V_A w and |w|^2
//   kg_rows_score_kernel  one workgroup per location: adds the shares, scores the lines and leaves the adjoint coefficients
//   kg_mix_kernel     w'_m = cw_m w_m + sum_i cv_mi V_A[i]: by linearity L^-T w'_m = cw_m beta_x + sum_i cv_mi beta_{a_i}, so the
//                     rows path's UNCHANGED backward pass delivers the whole adjoint of the training-side Jacobian in one read of L^-1
//   kg_close_kernel   over the training points: J(x)^T (cm alpha + L^-T w') and the cross terms dk(x, a_i)/dx (qei_close_kernel's geometry)
#include "rows_body.h"
#include "../../include/gphip.h"

#define KG_LINES (GP_KG_MAX_A + 1)
static_assert(GP_KG_MAX_A == 256 && KG_STATE_STRIDE >= GP_KG_MAX_A + 2, "a workgroup's thread per discretisation point; the state row takes the coefficients");

struct KgLines {   // a workgroup's LDS for one location: 257 lines x (a, b, p, q) + the reduction = 10 KB
    double a[KG_LINES], b[KG_LINES], p[KG_LINES], q[KG_LINES];
    double red[256];
};

// the floor of gpmodel.py:99 on the de-normalised latent variance, and the predictive standard deviation of the observation
__device__ __forceinline__ double kg_vfloor(double var, double ys2) { return fmax(var * ys2, 1e-10); }
__device__ __forceinline__ double kg_sd(double vf, double ys2, double noise) { return sqrt(vf + ys2 * noise); }

__device__ __forceinline__ double kg_tree(KgLines &L, double v) {   // sum over the workgroup's 256 threads, fixed tree; all get it
    const int t = threadIdx.x;
    __syncthreads();
    L.red[t] = v;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) L.red[t] += L.red[t + h];
        __syncthreads();
    }
    return L.red[0];
}

// The envelope of the n lines (L.a, L.b), n <= KG_LINES, called by all 256 threads behind a barrier that made the lines visible.
// Leaves p_i, q_i in L.p, L.q, the index of the lowest intercept (lowest index on a tie) in jstar, and returns
// sum_i (a~_i p_i + b_i q_i) = -KG in every thread.
__device__ __forceinline__ double kg_envelope(KgLines &L, int n, int &jstar) {
    const int t = threadIdx.x;
    double amin = L.a[0];
    int js = 0;
    for (int j = 1; j < n; ++j) {   // every thread walks the same words: one LDS address per step
        const double aj = L.a[j];
        if (aj < amin) {
            amin = aj;
            js = j;
        }
    }
    jstar = js;
    double part = 0.0;
    for (int i = t; i < n; i += 256) {
        const double ai = L.a[i] - amin, bi = L.b[i];
        double lo = -INFINITY, hi = INFINITY;
        bool dead = false;
        for (int j = 0; j < n; ++j) {
            const double aj = L.a[j] - amin, d = bi - L.b[j];
            const double z = (aj - ai) / d;
            if (d > 0.0) hi = fmin(hi, z);
            else if (d < 0.0) lo = fmax(lo, z);
            else if (j != i) dead |= (aj < ai) || (aj == ai && j < i);   // parallel: the lower one; identical: the lowest index
        }
        double p = 0.0, q = 0.0;
        if (!dead && lo < hi) {
            const double r2 = 0.70710678118654752440, c = 0.39894228040143267794;
            p = (hi <= 0.0) ? 0.5 * (erfc(-hi * r2) - erfc(-lo * r2)) : 0.5 * (erfc(lo * r2) - erfc(hi * r2));
            q = c * (exp(-0.5 * lo * lo) - exp(-0.5 * hi * hi));
        }
        L.p[i] = p;
        L.q[i] = q;
        part += ai * p + bi * q;   // (n <= 257: thread 0 alone takes a second line, line 256 after line 0)
    }
    return kg_tree(L, part);
}

// ---- table --------------------------------------------------------------------------------------------------------------------------
// C [mc, ldc] latent covariance candidate x discretisation point; mean / var [mc] the candidates' latent posterior, var without noise;
// muA [A] the points' latent means.  out [mc] = +KG.
__global__ __launch_bounds__(256) void kg_score_kernel(const double *__restrict__ C, long ldc, const double *__restrict__ mean,
                                                        const double *__restrict__ var, double y_std, double noise, int A,
                                                        const double *__restrict__ muA, double *__restrict__ out) {
    __shared__ KgLines L;
    const int t = threadIdx.x;
    const long c = blockIdx.x;
    const double ys2 = y_std * y_std;
    const double vf = kg_vfloor(var[c], ys2), sd = kg_sd(vf, ys2, noise);
    for (int i = t; i < A; i += 256) {
        L.a[i] = y_std * muA[i];
        L.b[i] = ys2 * C[c * ldc + i] / sd;
    }
    if (t == 0) {
        L.a[A] = y_std * mean[c];
        L.b[A] = vf / sd;
    }
    __syncthreads();
    int jstar;
    const double s = kg_envelope(L, A + 1, jstar);
    if (t == 0) out[c] = -s;
}

void launch_kg_score(hipStream_t s, const double *C, long ldc, const double *mean, const double *var, long mc, double y_std,
                     double noise, int A, const double *muA, double *out) {
    if (mc <= 0) return;
    GP_LAUNCH(kg_score_kernel, dim3((unsigned)mc), dim3(256), 0, s, C, ldc, mean, var, y_std, noise, A, muA, out);
}

// ---- a handful of locations behind the fused rows path's forward pass ----------------------------------------------------------------
// The forward pass left w_m = L^-1 k*_m as chunk partials wpart[C][m][n] and the mean's terms meanpart[C][m] (rows_body.h).
// kg_rows_kernel (es_rows_kernel's geometry): workgroup b takes the KG_ROWS_NB entries of w from n0 = b KG_ROWS_NB, sums their partials
// in chunk order, then cpart[b][m][i] = sum_n V_A[i, n] w_m[n] and the |w_m|^2 share, each with one writer.
// kg_rows_score_kernel: ONE WORKGROUP PER LOCATION (the envelope's A^2 quotients of eight locations side by side, not one after the
// other) adds the shares in workgroup order, forms the lines and scores them with the table kernel's arithmetic.  Results: -KG at
// [2 MV + m], the acquisition's place in the rows layout; for a gradient call the state row of location m
//   [cv_i = y_std^2 q_i / sd, i < A | cw = 2 y_std^2 (q_A / sd - sum_i q_i b_i / (2 sd^2)), 0 where the floor holds | cm = ([j* = A] - p_A) y_std]
// so that dKG/dx = J^T (cm alpha + L^-T (cw w + sum_i cv_i V_A[i])) - sum_i cv_i dk(x, a_i)/dx.  The M workgroups arrive at the pass's
// counter; in a value call the last of them writes the ticket.
#define KG_ROWS_NB 256
#define KG_CP_STRIDE (ROWS_WIDE_M * (GP_KG_MAX_A + 1))   // a workgroup's shares: [m][i], then the |w_m|^2
__global__ __launch_bounds__(256) void kg_rows_kernel(int M, int A, const double *__restrict__ VA, long Npad,
                                                       const double *__restrict__ wpart, int MV, double *__restrict__ cpart) {
    __shared__ double w_s[ROWS_WIDE_M][KG_ROWS_NB];
    __shared__ double red[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const unsigned b = blockIdx.x;
    const long n = (long)b * KG_ROWS_NB + t;
    double *mine = cpart + (long)b * KG_CP_STRIDE;
    {
        const bool live = n < Npad;
        const int nch = rw_nch((int)((live ? n : 0) / GP_TILE));
        for (int m = 0; m < M; ++m) {
            double s = 0.0;
            if (live)
                for (int C = 0; C < nch; ++C) s += wpart[((long)C * MV + m) * Npad + n];
            w_s[m][t] = s;
            const double q = rw_block_sum(s * s, red);
            if (t == 0) mine[ROWS_WIDE_M * GP_KG_MAX_A + m] = q;
        }
    }
    __syncthreads();
    for (int i = wave; i < A; i += 4) {
        const double *row = VA + (long)i * Npad + (long)b * KG_ROWS_NB;
        double v[KG_ROWS_NB / 64];
#pragma unroll
        for (int q = 0; q < KG_ROWS_NB / 64; ++q) v[q] = ((long)b * KG_ROWS_NB + lane + 64 * q < Npad) ? row[lane + 64 * q] : 0.0;
        for (int m = 0; m < M; ++m) {
            double a = 0.0;
#pragma unroll
            for (int q = 0; q < KG_ROWS_NB / 64; ++q) a = fma(v[q], w_s[m][lane + 64 * q], a);
            a = rw_wave_sum(a);
            if (lane == 0) mine[m * GP_KG_MAX_A + i] = a;
        }
    }
}

__global__ __launch_bounds__(256) void kg_rows_score_kernel(RowsX rx, KernParams kp, const double *__restrict__ Xa, int A,
                                                             const double *__restrict__ muA, const double *__restrict__ cpart, unsigned nblk,
                                                             const double *__restrict__ meanpart, int nmean, int MV, double kss,
                                                             double noise, double y_std, int want_grad, double *__restrict__ state,
                                                             unsigned int *counter, unsigned int counter_base, double *out, double ticket) {
    __shared__ KgLines L;
    __shared__ double var_s, mean_s;
    const int t = threadIdx.x;
    const int m = blockIdx.x, D = kp.D;
    if (t == 0) {
        double s = 0.0;
        for (unsigned k = 0; k < nblk; ++k) s += cpart[(long)k * KG_CP_STRIDE + ROWS_WIDE_M * GP_KG_MAX_A + m];
        var_s = kss - s;
        double mu = 0.0;
        for (int C = 0; C < nmean; ++C) mu += meanpart[C * MV + m];
        mean_s = mu;
    }
    __syncthreads();
    const double ys2 = y_std * y_std;
    const double vf = kg_vfloor(var_s, ys2), sd = kg_sd(vf, ys2, noise);
    for (int i = t; i < A; i += 256) {
        // k(x_m, a_i): the arithmetic of the forward pass's k* (inputs divided first, squares summed in dimension order)
        double acc = 0.0;
        for (int d = 0; d < D; ++d) {
            const double df = rx.xs[m * D + d] / kp.ls[d] - Xa[i * D + d] / kp.ls[d];
            acc = fma(df, df, acc);
        }
        double s = 0.0;
        for (unsigned k = 0; k < nblk; ++k) s += cpart[(long)k * KG_CP_STRIDE + m * GP_KG_MAX_A + i];
        L.a[i] = y_std * muA[i];
        L.b[i] = ys2 * (gp_k_of_r2(kp.kernel, kp.variance, acc) - s) / sd;
    }
    if (t == 0) {
        L.a[A] = y_std * mean_s;
        L.b[A] = vf / sd;
    }
    __syncthreads();
    int jstar;
    const double s = kg_envelope(L, A + 1, jstar);
    if (t == 0) out[2 * MV + m] = s;   // -KG
    if (want_grad) {
        double part = 0.0;
        for (int i = t; i < A + 1; i += 256) part += L.q[i] * L.b[i];
        const double qb = kg_tree(L, part);
        double *st = state + (long)m * KG_STATE_STRIDE;
        for (int i = t; i < A; i += 256) st[i] = ys2 * L.q[i] / sd;
        if (t == 0) {
            const bool floored = !(var_s * ys2 > 1e-10);
            st[GP_KG_MAX_A] = floored ? 0.0 : 2.0 * ys2 * (L.q[A] / sd - qb / (2.0 * sd * sd));
            st[GP_KG_MAX_A + 1] = ((jstar == A ? 1.0 : 0.0) - L.p[A]) * y_std;
        }
    }
    if (t == 0) {
        __threadfence_system();   // this location's result is out before the arrival
        const bool last = atomicAdd(counter, 1u) - counter_base == gridDim.x - 1;   // (unsigned: wraps with the base)
        if (last && !want_grad) {
            __threadfence_system();
            out[ROWS_OUT_DOUBLES] = ticket;   // this pass is complete (the host checks the ticket behind the results)
        }
    }
}

unsigned kg_rows_grid(long Npad) { return (unsigned)((Npad + KG_ROWS_NB - 1) / KG_ROWS_NB); }
size_t kg_rows_part_elems(long Npad) { return (size_t)kg_rows_grid(Npad) * KG_CP_STRIDE; }

void launch_kg_rows(hipStream_t s, const RowsX &rx, const KernParams &kp, const double *Xa, int A, const double *VA, const double *muA,
                    long Npad, const RowsWork &w, double *cpart, double kss, double noise, double y_std, int want_grad, double *state,
                    const PassReport &r) {
    const int nt = (int)(Npad / GP_TILE), MV = rows_layout(rx.M);
    GP_LAUNCH(kg_rows_kernel, dim3(kg_rows_grid(Npad)), dim3(256), 0, s, rx.M, A, VA, Npad, w.wpart, MV, cpart);
    GP_LAUNCH(kg_rows_score_kernel, dim3((unsigned)rx.M), dim3(256), 0, s, rx, kp, Xa, A, muA, cpart, kg_rows_grid(Npad), w.meanpart,
              rw_nch(nt - 1), MV, kss, noise, y_std, want_grad, state, r.counter, r.base, r.out, r.ticket);
}

// ---- the adjoint's mix ---------------------------------------------------------------------------------------------------------------
// One thread per training row n: w_m[n] from the chunk partials in chunk order, w'_m[n] = cw_m w_m[n] + sum_i cv_mi V_A[i, n] with i in
// index order by fma, written back as chunk 0 of wpart with zeros in the row's other chunks -- what the backward pass then sums.
__global__ __launch_bounds__(256) void kg_mix_kernel(double *wpart, long Npad, long N, int M, int MV, const double *__restrict__ VA, int A,
                                                      const double *__restrict__ state) {
    __shared__ double cv_s[ROWS_WIDE_M][GP_KG_MAX_A];
    __shared__ double cw_s[ROWS_WIDE_M];
    const int t = threadIdx.x;
    for (int e = t; e < M * GP_KG_MAX_A; e += 256) {
        const int m = e / GP_KG_MAX_A, i = e - m * GP_KG_MAX_A;
        cv_s[m][i] = i < A ? state[(long)m * KG_STATE_STRIDE + i] : 0.0;
    }
    if (t < M) cw_s[t] = state[(long)t * KG_STATE_STRIDE + GP_KG_MAX_A];
    __syncthreads();
    const long n = (long)blockIdx.x * 256 + t;
    if (n >= Npad) return;
    const int nch = rw_nch((int)(n / GP_TILE));
    double acc[ROWS_WIDE_M];
#pragma unroll
    for (int m = 0; m < ROWS_WIDE_M; ++m) {
        double s = 0.0;
        if (m < M)
            for (int C = 0; C < nch; ++C) s += wpart[((long)C * MV + m) * Npad + n];
        acc[m] = m < M ? cw_s[m] * s : 0.0;
    }
    if (n < N) {
        for (int i = 0; i < A; ++i) {
            const double v = VA[(long)i * Npad + n];
#pragma unroll
            for (int m = 0; m < ROWS_WIDE_M; ++m) acc[m] = fma(cv_s[m][i], v, acc[m]);
        }
    }
#pragma unroll
    for (int m = 0; m < ROWS_WIDE_M; ++m) {
        if (m < M) {
            wpart[(long)m * Npad + n] = n < N ? acc[m] : 0.0;
            for (int C = 1; C < nch; ++C) wpart[((long)C * MV + m) * Npad + n] = 0.0;
        }
    }
}

void launch_kg_mix(hipStream_t s, int M, long N, long Npad, const RowsWork &w, const double *VA, int A, const double *state) {
    GP_LAUNCH(kg_mix_kernel, dim3((unsigned)((Npad + 255) / 256)), dim3(256), 0, s, w.wpart, Npad, N, M, rows_layout(M), VA, A, state);
}

// ---- the closing pass over the training points -----------------------------------------------------------------------------------------
// grid = rows_finish_grid(N) workgroups of 256 threads, 64 training rows each (rows_finish_body's geometry): t_m[n] = (L^-T w'_m)[n] from
// the backward pass's row-block partials, then location m (wave m % 4) takes row n through ONE gradients_X sum with the weight
// g (cm_m alpha_n + t_m[n]).  The last workgroup to arrive adds the workgroups' sums in eight interleaved slices, subtracts the cross
// terms sum_i cv_mi dk(x_m, a_i)/dx, i in index order, and writes the NEGATED gradient at the rows layout's dacq and the ticket.
__global__ __launch_bounds__(256) void kg_close_kernel(RowsX rx, KernParams kp, const double *X, long N, const double *alpha,
                                                        const double *bpart, long Npad, int MV, int nt, int rbh,
                                                        const double *__restrict__ Xa, int A, const double *__restrict__ state,
                                                        double *gpart, unsigned int *counter, unsigned int counter_base, double *out,
                                                        double ticket) {
    constexpr int Q = ROWS_WIDE_M;
    __shared__ double xs_s[ROWS_MAX_XS];
    __shared__ double part_s[4][Q][64];
    __shared__ double b_s[Q][64];
    __shared__ double cm_s[Q];
    __shared__ double fin_s[8][ROWS_MAX_XS];
    __shared__ double res_s[ROWS_MAX_XS];
    __shared__ double wg_s[Q][GP_KG_MAX_A];
    __shared__ int last_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int D = kp.D, M = rx.M;
    const long n = (long)blockIdx.x * 64 + lane;
    const bool live = n < N;
    const int nrb = nt * (GP_TILE / rbh);
    for (int i = tid; i < M * D; i += 256) xs_s[i] = rx.xs[i] / kp.ls[i % D];
    if (tid < M) cm_s[tid] = state[(long)tid * KG_STATE_STRIDE + GP_KG_MAX_A + 1];
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
        const double c = live ? gv * (cm_s[i] * a + b_s[i][lane]) : 0.0;
        for (int d = 0; d < D; ++d) {
            const double dq = live ? xs_s[i * D + d] - X[n * D + d] / kp.ls[d] : 0.0;
            const double v = rw_wave_sum(c * dq);
            if (lane == 0) gpart[(long)blockIdx.x * RW_GROW + i * D + d] = v;
        }
    }
    __threadfence();
    __syncthreads();
    if (tid == 0) last_s = (atomicAdd(counter, 1u) - counter_base == gridDim.x - 1) ? 1 : 0;   // (unsigned: wraps with the base)
    __syncthreads();
    if (!last_s) return;
    __threadfence();
    const int nval = M * D;
    for (int idx = tid; idx < 8 * nval; idx += 256) {
        const int v = idx % nval, j = idx / nval;
        fin_s[j][v] = rw_strided_sum(gpart + v, RW_GROW, j, 8, (int)gridDim.x);
    }
    // the cross terms' weights cv_mi g(r(x_m, a_i)), one (m, i) per step of a thread
    for (int e = tid; e < M * A; e += 256) {
        const int m = e / A, i = e - m * A;
        double r2 = 0.0;
        for (int d = 0; d < D; ++d) {
            const double df = xs_s[m * D + d] - Xa[i * D + d] / kp.ls[d];
            r2 = fma(df, df, r2);
        }
        double kv, gv;
        gp_k_and_g(kp.kernel, kp.variance, r2, kv, gv);
        if (r2 == 0.0) gv = 0.0;
        wg_s[m][i] = state[(long)m * KG_STATE_STRIDE + i] * gv;
    }
    __syncthreads();
    for (int v = tid; v < nval; v += 256) {
        double s = 0.0;
        for (int j = 0; j < 8; ++j) s += fin_s[j][v];
        res_s[v] = s;
    }
    __syncthreads();
    const int MVD = MV * D;
    for (int v = tid; v < nval; v += 256) {
        const int m = v / D, d = v % D;
        double cross = 0.0;
        for (int i = 0; i < A; ++i) cross = fma(wg_s[m][i], xs_s[m * D + d] - Xa[i * D + d] / kp.ls[d], cross);
        out[3 * MV + 2 * MVD + v] = -((res_s[v] - cross) / kp.ls[d]);   // (x - x') / l^2 = scaled difference / l
    }
    __syncthreads();
    __threadfence_system();
    if (tid == 0) out[ROWS_OUT_DOUBLES] = ticket;
}

void launch_kg_close(hipStream_t s, const RowsX &rx, const KernParams &kp, const double *X, long N, long Npad, const double *alpha,
                     const RowsWork &w, const double *Xa, int A, const double *state, const PassReport &r, unsigned counter_base) {
    const int nt = (int)(Npad / GP_TILE);
    GP_LAUNCH(kg_close_kernel, dim3(rows_finish_grid(N)), dim3(256), 0, s, rx, kp, X, N, alpha, w.bpart, Npad, rows_layout(rx.M), nt,
              rows_block_height(nt), Xa, A, state, w.gpart, r.counter, counter_base, r.out, r.ticket);
}
