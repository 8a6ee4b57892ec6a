// Noisy expected improvement (Letham, Karrer, Ottoni & Bakshy 2019): EI averaged over S <= NEI_SPAD fantasies of the noiseless
// function values at the training inputs (include/gphip.h has the definitions; api_nei.hip and api_rows.hip the sequences).  Always
// true fp64; every sum has a fixed order, no atomics but the rows path's arrival counter.
//
// Kernels:
//   nei_lz_kernel          g_s = L0 z_s for all S at once: ONE read of the factor's lower triangle, a wave per row, a lane per fantasy
//   nei_assemble_kernel    mode 0: b = y - sd e into F and the residual b - g in g's place; mode 1: F -= dd V
//   nei_colmin_kernel      fstar_s = min_i F_is, one workgroup per fantasy, fixed tree
//   nei_same_x_kernel      the two handles' inputs compared entry by entry
//   nei_score_kernel       table: one thread per candidate over its S means, the S EIs in index order
//   nei_rows_kernel        behind the fused rows path's forward pass (kg_rows_kernel's geometry): the shares of k . a_s and |w|^2
//   nei_rows_score_kernel  one workgroup per location: adds the shares in workgroup order, scores, leaves the adjoint's state row
// The gradient's mix and closing pass are the knowledge gradient's (kg_mix_kernel with U = L0^-1 F in V_A's place, kg_close_kernel
// without cross terms): the state row has their layout.
#include "rows_body.h"
#include "../../include/gphip.h"

static_assert(NEI_SPAD == GP_NEI_MAX_S && NEI_SPAD == 64, "a lane per fantasy");
static_assert(NEI_SPAD <= GP_KG_MAX_A, "the state row of the knowledge gradient takes the S coefficients");
static_assert(GP_NEI_MAX_ROWS == ROWS_WIDE_M, "a wide pass takes GP_NEI_MAX_ROWS locations");

// ---- the fantasies ------------------------------------------------------------------------------------------------------------------
// Wave = row i of L, lane = fantasy s.  The row is read 64 entries at a time, one per lane, and handed round by lane index; Zt's row j
// is one coalesced load.  acc runs over j = 0 .. i in order by fma: a fantasy's bits depend on no other fantasy.  L is read once; what
// bounds the kernel is the 512-byte row of Zt every wave re-reads per j from L2 (N^2 / 2 of them) and the final store, 64 rows of G a
// stride ldg apart.  Once per model update (DESIGN.md has the figures).
__global__ __launch_bounds__(256) void nei_lz_kernel(const double *__restrict__ L, long ldl, long N, const double *__restrict__ Zt,
                                                      double *__restrict__ G, long ldg) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;   // (a whole wave)
    const double *row = L + i * ldl;
    double acc = 0.0;
    for (long j0 = 0; j0 <= i; j0 += 64) {
        const long j = j0 + lane;
        const double lv = j <= i ? row[j] : 0.0;
        const int kmax = (int)min(64L, i - j0 + 1);
        for (int k = 0; k < kmax; ++k) acc = fma(__shfl(lv, k), Zt[(j0 + k) * NEI_SPAD + lane], acc);
    }
    G[(long)lane * ldg + i] = acc;
}
void launch_nei_lz(hipStream_t s, const double *L, long ldl, long N, const double *Zt, double *G, long ldg) {
    GP_LAUNCH(nei_lz_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, L, ldl, N, Zt, G, ldg);
}

__global__ __launch_bounds__(256) void nei_assemble_kernel(int mode, long N, const double *__restrict__ Y, const double *__restrict__ Em,
                                                            double sd, double dd, double *__restrict__ G, const double *__restrict__ V,
                                                            double *__restrict__ F, long ld) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const long at = (long)blockIdx.y * ld + i;
    if (mode == 0) {
        const double b = fma(-sd, Em[at], Y[i]);
        F[at] = b;
        G[at] = b - G[at];
    } else {
        F[at] = fma(-dd, V[at], F[at]);
    }
}
void launch_nei_assemble(hipStream_t s, int mode, int S, long N, const double *Y, const double *Em, double sd, double dd, double *G,
                         const double *V, double *F, long ld) {
    GP_LAUNCH(nei_assemble_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)S), dim3(256), 0, s, mode, N, Y, Em, sd, dd, G, V, F, ld);
}

__global__ __launch_bounds__(256) void nei_colmin_kernel(const double *__restrict__ F, long ld, long N, double *__restrict__ fstar) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    const double *row = F + (long)blockIdx.x * ld;
    double v = INFINITY;
    for (long i = t; i < N; i += 256) v = fmin(v, row[i]);
    red[t] = v;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) red[t] = fmin(red[t], red[t + h]);
        __syncthreads();
    }
    if (t == 0) fstar[blockIdx.x] = red[0];
}
void launch_nei_colmin(hipStream_t s, const double *F, long ld, long N, int S, double *fstar) {
    GP_LAUNCH(nei_colmin_kernel, dim3((unsigned)S), dim3(256), 0, s, F, ld, N, fstar);
}

__global__ __launch_bounds__(256) void nei_same_x_kernel(const double *__restrict__ Xa, const double *__restrict__ Xb, long n, int *flag) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n && Xa[i] != Xb[i]) flag[0] = 1;   // (every writer writes the same word)
}
void launch_nei_same_x(hipStream_t s, const double *Xa, const double *Xb, long n, int *flag) {
    GP_LAUNCH(nei_same_x_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, Xa, Xb, n, flag);
}

// ---- scoring ------------------------------------------------------------------------------------------------------------------------
// The twin's predictive standard deviation as acq_terms forms it, and whether the variance's floor holds
__device__ __forceinline__ double nei_sd(double var, double y_std, bool &floored) {
    double v = var * (y_std * y_std);
    floored = v < 1e-10;
    v = floored ? 1e-10 : v;
    double s = sqrt(v);
    if (s < 1e-10) s = 1e-10;
    return s;
}
// One fantasy's share: acq_terms' EI arithmetic with the fantasy's own incumbent.  No product is contracted into an fma: the table
// and the rows route run the operations as written.
__device__ __forceinline__ void nei_term(double m_s, double fstar_s, double par, double y_mean, double y_std, double s, double &ei,
                                         double &Phi, double &phi) {
#pragma clang fp contract(off)
    const double mu = m_s * y_std + y_mean;
    const double t = fstar_s * y_std + y_mean;
    const double u = (t - mu - par) / s;
    phi = exp(-0.5 * u * u) / 2.50662827463100050241576528481105;
    Phi = 0.5 * erfc(-u / 1.41421356237309504880168872420970);
    ei = s * (u * Phi + phi);
}

__global__ __launch_bounds__(256) void nei_score_kernel(const double *__restrict__ mtab, const double *__restrict__ var, long M, int S,
                                                         const double *__restrict__ fstar, double par, double y_mean, double y_std,
                                                         double *__restrict__ out) {
    __shared__ double fs[NEI_SPAD];
    if (threadIdx.x < S) fs[threadIdx.x] = fstar[threadIdx.x];
    __syncthreads();
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    bool floored;
    const double s = nei_sd(var[i], y_std, floored);
    double sum = 0.0;
    for (int k = 0; k < S; ++k) {
        double ei, Phi, phi;
        nei_term(mtab[(long)k * M + i], fs[k], par, y_mean, y_std, s, ei, Phi, phi);
        sum += ei;
    }
    out[i] = sum / (double)S;
}
void launch_nei_score(hipStream_t s, const double *mtab, const double *var, long M, int S, const double *fstar, double par,
                      double y_mean, double y_std, double *out) {
    if (M <= 0) return;
    GP_LAUNCH(nei_score_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, mtab, var, M, S, fstar, par, y_mean, y_std, out);
}

// ---- a handful of locations behind the fused rows path's forward pass ----------------------------------------------------------------
// The forward pass left w_m = L0^-1 k*_m as chunk partials wpart[C][m][n] (rows_body.h).  nei_rows_kernel: workgroup b takes the
// NEI_ROWS_NB training rows from n0 = b NEI_ROWS_NB: the |w_m|^2 share from the partials in chunk order, k*_m[n] by the forward
// pass's arithmetic (inputs divided first, squares summed in dimension order), then cpart[b][m][s] = sum_n A0[s, n] k*_m[n], wave
// s % 4 per fantasy, each with one writer.  nei_rows_score_kernel: ONE WORKGROUP PER LOCATION adds the shares in workgroup order,
// thread s < S for fantasy s, and thread 0 adds the S terms in index order.  Results: -NEI at [2 MV + m]; for a gradient call the
// state row of location m (gphip_internal.h).  The M workgroups arrive at the pass's counter; in a value call the last of them
// writes the ticket.  Nothing in a location's arithmetic looks at M, MV or its slot.
#define NEI_ROWS_NB 256
#define NEI_CP_STRIDE (ROWS_WIDE_M * (NEI_SPAD + 1))   // a workgroup's shares: [m][s], then the |w_m|^2
__global__ __launch_bounds__(256) void nei_rows_kernel(RowsX rx, KernParams kp, const double *__restrict__ X, long N, long Npad,
                                                        const double *__restrict__ A0, int S, const double *__restrict__ wpart, int MV,
                                                        double *__restrict__ cpart) {
    __shared__ double k_s[ROWS_WIDE_M][NEI_ROWS_NB];
    __shared__ double xs_s[ROWS_MAX_XS];
    __shared__ double red[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const unsigned b = blockIdx.x;
    const int D = kp.D, M = rx.M;
    const long n = (long)b * NEI_ROWS_NB + t;
    double *mine = cpart + (long)b * NEI_CP_STRIDE;
    for (int i = t; i < M * D; i += 256) xs_s[i] = rx.xs[i] / kp.ls[i % D];
    __syncthreads();
    {
        const bool pad = n < Npad, live = n < N;
        const int nch = rw_nch((int)((pad ? n : 0) / GP_TILE));
        for (int m = 0; m < M; ++m) {
            double s = 0.0;
            if (pad)
                for (int C = 0; C < nch; ++C) s += wpart[((long)C * MV + m) * Npad + n];
            const double q = rw_block_sum(s * s, red);
            if (t == 0) mine[ROWS_WIDE_M * NEI_SPAD + m] = q;
            double acc = 0.0;
            if (live)
                for (int d = 0; d < D; ++d) {
                    const double df = xs_s[m * D + d] - X[n * D + d] / kp.ls[d];
                    acc = fma(df, df, acc);
                }
            k_s[m][t] = live ? gp_k_of_r2(kp.kernel, kp.variance, acc) : 0.0;
        }
    }
    __syncthreads();
    for (int i = wave; i < S; i += 4) {
        const double *row = A0 + (long)i * Npad + (long)b * NEI_ROWS_NB;
        double v[NEI_ROWS_NB / 64];
#pragma unroll
        for (int q = 0; q < NEI_ROWS_NB / 64; ++q) v[q] = ((long)b * NEI_ROWS_NB + lane + 64 * q < N) ? row[lane + 64 * q] : 0.0;
        for (int m = 0; m < M; ++m) {
            double a = 0.0;
#pragma unroll
            for (int q = 0; q < NEI_ROWS_NB / 64; ++q) a = fma(v[q], k_s[m][lane + 64 * q], a);
            a = rw_wave_sum(a);
            if (lane == 0) mine[m * NEI_SPAD + i] = a;
        }
    }
}

__global__ __launch_bounds__(64) void nei_rows_score_kernel(int S, const double *__restrict__ fstar, const double *__restrict__ cpart,
                                                             unsigned nblk, int MV, double kss, double noise_add, double par,
                                                             double y_mean, double y_std, int want_grad, double *__restrict__ state,
                                                             unsigned int *counter, unsigned int counter_base, double *out,
                                                             double ticket) {
    __shared__ double ei_s[NEI_SPAD], Phi_s[NEI_SPAD], phi_s[NEI_SPAD];
    __shared__ double sd_s;
    __shared__ int floor_s;
    const int t = threadIdx.x;
    const int m = blockIdx.x;
    if (t == 0) {
        double q = 0.0;
        for (unsigned k = 0; k < nblk; ++k) q += cpart[(long)k * NEI_CP_STRIDE + ROWS_WIDE_M * NEI_SPAD + m];
        bool floored;
        sd_s = nei_sd((kss - q) + noise_add, y_std, floored);
        floor_s = floored ? 1 : 0;
    }
    __syncthreads();
    const double sd = sd_s;
    if (t < S) {
        double ms = 0.0;
        for (unsigned k = 0; k < nblk; ++k) ms += cpart[(long)k * NEI_CP_STRIDE + m * NEI_SPAD + t];
        double ei, Phi, phi;
        nei_term(ms, fstar[t], par, y_mean, y_std, sd, ei, Phi, phi);
        ei_s[t] = ei;
        Phi_s[t] = Phi;
        phi_s[t] = phi;
    }
    __syncthreads();
    if (want_grad) {
        double *st = state + (long)m * KG_STATE_STRIDE;
        if (t < S) st[t] = -(y_std * (Phi_s[t] / (double)S));
    }
    if (t == 0) {
        double sum = 0.0, c = 0.0;
        for (int k = 0; k < S; ++k) {
            sum += ei_s[k];
            c += phi_s[k];
        }
        out[2 * MV + m] = -(sum / (double)S);
        if (want_grad) {
            double *st = state + (long)m * KG_STATE_STRIDE;
            c = c / (double)S;
            st[GP_KG_MAX_A] = floor_s ? 0.0 : -(c * (y_std * y_std) / sd);
            st[GP_KG_MAX_A + 1] = 0.0;
        }
        __threadfence_system();   // this location's result is out before the arrival
        const bool last = atomicAdd(counter, 1u) - counter_base == gridDim.x - 1;   // (unsigned: wraps with the base)
        if (last && !want_grad) {
            __threadfence_system();
            out[ROWS_OUT_DOUBLES] = ticket;   // this pass is complete (the host checks the ticket behind the results)
        }
    }
}

unsigned nei_rows_grid(long Npad) { return (unsigned)((Npad + NEI_ROWS_NB - 1) / NEI_ROWS_NB); }
size_t nei_rows_part_elems(long Npad) { return (size_t)nei_rows_grid(Npad) * NEI_CP_STRIDE; }

int launch_nei_rows(hipStream_t s, const RowsX &rx, const KernParams &kp, const double *X, long N, long Npad, const double *A0, int S,
                     const double *fstar, const RowsWork &w, double *cpart, double kss, double noise_add, double par, double y_mean,
                     double y_std, int want_grad, double *state, const PassReport &r) {
    const int MV = rows_layout(rx.M);
    GP_LAUNCH(nei_rows_kernel, dim3(nei_rows_grid(Npad)), dim3(256), 0, s, rx, kp, X, N, Npad, A0, S, w.wpart, MV, cpart);
    GP_LAUNCH(nei_rows_score_kernel, dim3((unsigned)rx.M), dim3(64), 0, s, S, fstar, cpart, nei_rows_grid(Npad), MV, kss, noise_add, par,
              y_mean, y_std, want_grad, state, r.counter, r.base, r.out, r.ticket);
    return 2;
}
