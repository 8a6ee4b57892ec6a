// Internal declarations shared by the gphip translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <string>
#include <vector>

#define GP_TILE 128          // tile edge of every blocked algorithm (rows/cols per workgroup tile)
#define GP_MAX_RHS 128       // RHS rows carried below the matrix (one tile)

typedef double double4_t __attribute__((ext_vector_type(4)));
typedef double double2_t __attribute__((ext_vector_type(2)));

// ---- launch / stream-operation checks ---------------------------------------------------------------------------------
// A refused kernel launch (resources, bad configuration) or a failed event record / stream wait reports through the HIP
// call's return value only; the launch_* helpers return void and sit many frames below the entry point.  Every launch and
// every stream-ordering call therefore NOTES its status in a per-thread slot (the first failure wins), and the entry
// points read that slot where they synchronise (GP_SYNC in api_internal.h): a failure anywhere in the call becomes
// GP_ERR_HIP with the kernel / call named, never a success over unwritten results.
void gp_note_hip(hipError_t e, const char *what, const char *file, int line);
#define GP_NOTE(call) gp_note_hip((call), #call, __FILE__, __LINE__)
#define GP_LAUNCH(kernel, grid, block, lds, stream, ...)                                   \
    do {                                                                                   \
        (void)hipGetLastError(); /* a stale status of an earlier, handled call is not this launch's */ \
        hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);                 \
        gp_note_hip(hipGetLastError(), #kernel, __FILE__, __LINE__);                       \
    } while (0)

// ---- kernel parameters of the stationary covariance (device copy) ----------
#define GP_MAX_D 64
struct KernParams {
    int kernel;            // GP_KERNEL_*
    int D;
    double variance;
    double ls[GP_MAX_D];       // lengthscale per dimension (iso: all equal)
    // the fork's "Gower" mixed-variable kernel (GPy/GPy/kern/src/stationary.py:116-135): K = prod_d k1(r_d),
    // r_d = |x_d - x'_d| / range_d for continuous dimensions, (x_d != x'_d) for discrete ones
    int gower;
    unsigned char gdisc[GP_MAX_D];  // 1: discrete dimension
    double gdiv[GP_MAX_D];          // staging divisor: range_d (continuous) or 1 (discrete)
};
// exp(x) for x <= 0 (the only arguments a stationary covariance has): n = rint(x log2 e), two-step reduction with the split
// ln 2, Taylor polynomial of degree 13 on |r| <= 0.347 (truncation 4e-18) in Horner form, scaling by v_ldexp_f64.  20
// instructions against ~35 of the library routine (no overflow / positive-range handling); at most 1 ulp from the exact value
// over [-745, 0] (20 M random arguments against an 80-bit reference on the host).  NaN stays NaN, -inf and x < -745.2 give 0.
__device__ __forceinline__ double gp_exp_nonpos(double x) {
    x = (x < -800.0) ? -800.0 : x;   // (a comparison, not fmax: NaN must pass)
    const double n = rint(x * 1.4426950408889634074);
    double r = fma(n, -6.93147180369123816490e-01, x);
    r = fma(n, -1.90821492927058770002e-10, r);
    double p = 1.0 / 6227020800.0;
    p = fma(p, r, 1.0 / 479001600.0);
    p = fma(p, r, 1.0 / 39916800.0);
    p = fma(p, r, 1.0 / 3628800.0);
    p = fma(p, r, 1.0 / 362880.0);
    p = fma(p, r, 1.0 / 40320.0);
    p = fma(p, r, 1.0 / 5040.0);
    p = fma(p, r, 1.0 / 720.0);
    p = fma(p, r, 1.0 / 120.0);
    p = fma(p, r, 1.0 / 24.0);
    p = fma(p, r, 1.0 / 6.0);
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    return ldexp(p, (int)n);
}

// the stationary covariance as a function of r^2, and with it g(r) = dK_dr(r) / r:
// RBF.K_of_r / dK_dr (rbf.py:50-54), Matern52.K_of_r / dK_dr (stationary.py:575-579), Matern32.K_of_r / dK_dr
// (stationary.py:478-482), Exponential.K_of_r / dK_dr (stationary.py:388-392).  The family is uniform across a launch, so
// the branches are scalar; the RBF and Matern-5/2 branches are the expressions they were before the other two came.
// g is finite at r = 0 for the first three.  The Exponential's dK_dr / r = -K / r is singular there, and the reference never
// divides by that zero: _inv_dist (stationary.py:251-258) is 0 where the distance is 0, so a coincident pair adds exactly 0
// to gradients_X and to the lengthscale gradients.  Hence g = 0 where r2 == 0, selected before the division (the divisor is
// never 0).  Away from 0 |g| is not bounded by |K| (it grows as 1 / r): every call site multiplies g by a scaled difference
// or by r^2, which brings the product back to O(K).
//
// The four families come in two pairs, GP_FAMILY_PAIR(kernel) = 0 (RBF, Matern-5/2) or 1 (Matern-3/2, Exponential).  The K-build
// tile kernels (kbuild.hip) and the LML-gradient tile kernels (grad.hip) take the pair as a template parameter chosen on the
// host: with all four families inlined kbuild_batch_kernel<8> and lml_grad_tile_kernel each lost one occupancy step
// (profiles/kernel_families_resources.txt), and pair 0 of the split compiles to the code it was before.  Every other caller
// keeps the run-time choice among the four.
#define GP_FAMILY_PAIR(kernel) ((kernel) >= 2 ? 1 : 0)
template <int PAIR>
__device__ __forceinline__ double gp_k_of_r2_pair(int kernel, double variance, double r2) {
    if (PAIR == 0) {
        if (kernel == 0) return variance * gp_exp_nonpos(-0.5 * r2);
        const double s5 = 2.23606797749978969640917366873128;  // sqrt(5)
        const double r = sqrt(r2);
        return variance * (1.0 + s5 * r + (5.0 / 3.0) * r2) * gp_exp_nonpos(-s5 * r);
    }
    const double r = sqrt(r2);
    if (kernel == 2) {
        const double s3 = 1.73205080756887729352744634150587;  // sqrt(3)
        return variance * (1.0 + s3 * r) * gp_exp_nonpos(-s3 * r);
    }
    return variance * gp_exp_nonpos(-r);
}
__device__ __forceinline__ double gp_k_of_r2(int kernel, double variance, double r2) {
    return GP_FAMILY_PAIR(kernel) ? gp_k_of_r2_pair<1>(kernel, variance, r2) : gp_k_of_r2_pair<0>(kernel, variance, r2);
}
template <int PAIR>
__device__ __forceinline__ void gp_k_and_g_pair(int kernel, double variance, double r2, double &k, double &g) {
    if (PAIR == 0) {
        if (kernel == 0) {
            k = variance * gp_exp_nonpos(-0.5 * r2);
            g = -k;  // dK_dr = -r k
        } else {
            const double s5 = 2.23606797749978969640917366873128;
            const double r = sqrt(r2);
            const double e = gp_exp_nonpos(-s5 * r);
            k = variance * (1.0 + s5 * r + (5.0 / 3.0) * r2) * e;
            g = -(5.0 / 3.0) * variance * (1.0 + s5 * r) * e;  // (10/3 r - 5 r - 5 sqrt5/3 r^2) e / r
        }
    } else if (kernel == 2) {
        const double s3 = 1.73205080756887729352744634150587;
        const double r = sqrt(r2);
        const double e = gp_exp_nonpos(-s3 * r);
        k = variance * (1.0 + s3 * r) * e;
        g = -3.0 * variance * e;  // dK_dr = -3 variance r e
    } else {
        const double r = sqrt(r2);
        k = variance * gp_exp_nonpos(-r);
        const bool zero = (r2 == 0.0);
        g = zero ? 0.0 : -k / (zero ? 1.0 : r);  // dK_dr = -k; the divisor is never 0
    }
}
__device__ __forceinline__ void gp_k_and_g(int kernel, double variance, double r2, double &k, double &g) {
    if (GP_FAMILY_PAIR(kernel)) gp_k_and_g_pair<1>(kernel, variance, r2, k, g);
    else gp_k_and_g_pair<0>(kernel, variance, r2, k, g);
}

// divisor used when staging inputs for a covariance evaluation
__host__ __device__ static inline double kp_div(const KernParams &kp, int d) { return kp.gower ? kp.gdiv[d] : kp.ls[d]; }

// ---- tile-set descriptor for the GEMM family ---------------------------------
// Enumerates output tiles (i, c): c in [c0, c1); rows i in [tri ? c : r0, r1).
struct TileSet {
    int r0, r1, c0, c1, tri;
};
static inline long tileset_count(const TileSet &t) {
    if (!t.tri) return (long)(t.r1 - t.r0) * (t.c1 - t.c0);
    long n = 0;
    for (int c = t.c0; c < t.c1; ++c) n += (t.r1 - c) > 0 ? (t.r1 - c) : 0;
    return n;
}

// C tile (i,c) at C + i*128*ldc + c*128
// A rows   at A + i*128*lda            (K columns)
// B rows   at B + (c*b_mul)*128*ldb    (K columns)
// mode 0: C = A B^T ; mode 1: C -= A B^T
struct GemmOpt {
    int k_tri = 0;      // k starts at the output row tile (A block upper-triangular) ...
    int k_sub = 0;      // ... minus k_sub tiles (the A / B pointers already sit at column tile k_sub)
    int k_end_tri = 0;  // k ends after column tile (tc - b_sub) (B block lower-triangular)
    int b_sub = 0;      // B row tile = (tc - b_sub) * b_mul
    int batch = 1;      // blockIdx.y instances with pointer strides sC, sA, sB (elements)
    int members = 1;    // ... of which this many are whole problems side by side (not parts of one): gemm() chooses the instance
                        // from one problem's tiles, batch / members of them, so that each gets the instance it would get alone
    long sC = 0, sA = 0, sB = 0;
    const short *tile_list = nullptr;  // device pointer, 2 shorts per tile, tileset_count(ts) tiles
    int stagger = 0;                   // odd-wave-slot workgroups start stagger * 1024 cycles late
    int small = 0;                     // 64x64 workgroup tiles (4 workgroups per 128-tile): latency-bound launches
    int waves8 = 0;                    // 128x128 tile on 8 waves (64x32 per wave, 4 waves/SIMD) instead of 4
    int sched = 0;                     // ... with the scheduled K loop (gemm_nt_sched_kernel; the paired twin keeps the plain one)
    int inplace = 0;                   // C aliases A (tile-local product): the 128-tile must stay in one workgroup
    int rows64 = 0;                    // 64-row strips of the 128-tile (two workgroups per tile; safe in place)
    int pair = 0;                      // k_end_tri, rectangular tile set, small tiles: column tiles paired for equal K
};
// Host-side construction of an L2-friendly order: the tile set is cut into S x S super-tiles; the
// list is dealt so that each XCD's contiguous run (see the remap in gemm.hip) walks whole super-tiles.
std::vector<short> build_tile_list(const TileSet &ts, int S);
void launch_gemm_nt(hipStream_t s, int mode, double *C, long ldc, const double *A, long lda,
                    const double *B, long ldb, int b_mul, int K, TileSet ts, const GemmOpt &o = GemmOpt());

// Factor the 128x128 diagonal tile t of A (row-major, lda) in place (lower) and write
// its inverse (row-major 128x128, lower, zero above) to invL + t*128*128.
// info: device int, 0 = ok, else 1-based global column of the first non-positive pivot.
void launch_potrf_tile(hipStream_t s, double *A, long lda, int t, double *invL, int *info, int nb = 1, long sA = 0, long sI = 0,
                       int sInfo = 0);
// The same for the diagonal tiles t and t + 1 in one launch, including L10 = A10 inv(L00)^T and A11 -= L10 L10^T between them.
void launch_potrf_pair(hipStream_t s, double *A, long lda, int t, double *invL, int *info);
// Both tile columns of the rows below a factored pair, one launch: for every 32-row strip of the row tiles [r0, r1)
//   X0 = A[., t] inv(L_tt)^T;  A[., t+1] -= X0 L[t+1, t]^T;  X1 = A[., t+1] inv(L_t+1,t+1)^T     (in place)
void launch_trsm2(hipStream_t s, double *A, long lda, int t, const double *invL, int r0, int r1);
void potrf_set_debug_lds(int bytes);   // test hook: dynamic LDS added to every diagonal-tile launch (a refused launch beyond ~9 KB)

// ---- launches that take members ---------------------------------------------------------------------------------------------
// The launchers with a trailing `nb` run nb independent problems ("members") side by side: member z at base + z * stride
// (blockIdx.z, or blockIdx.x for the one-workgroup kernels); the inputs and targets of member z are at X + z * sX, Y + z * sY
// (strides 0: the members share them).  One member (the default) is the single-member kernel with the
// values given on the host (kp, diag_add, v); several are its _batch twin, which runs the same body per member -- the per-tile
// arithmetic of the single launch -- and reads per-member values from device tables (kpt[z], diag_tab[z], v_tab[z]), kp then
// being the first member's: what selects the instance and the LDS size.  Only the launchers ask "one member or several".

// Ky lower tiles (incl. diagonal tiles in full) from X; padding rows get identity.  (Several members: lower tiles only.)
void launch_kbuild(hipStream_t s, double *A, long lda, const double *X, long N, long Npad, const KernParams &kp, double diag_add,
                   int full, int nb = 1, long sA = 0, const KernParams *kpt = nullptr, const double *diag_tab = nullptr, long sX = 0);
// RHS rows: A[(Npad + p)*lda + i] = Y[i*P + p] (zero for i >= N, and rows p >= P zero)
void launch_set_rhs(hipStream_t s, double *A, long lda, const double *Y, long N, long Npad, int P, int nb = 1, long sA = 0, long sY = 0);
// T[c*ldt + i] = k(xs_c, x_i) for c < M, i < N; zero in the padding.
// nb > 1: nb members in one launch, member z = blockIdx.z with its own block at T + z sT, its own second input set at X + z sX and
// parameters kpt[z] (device); Xs is shared, and kp (the first member's) picks the instance and the LDS size for all
void launch_cross_k(hipStream_t s, double *T, long ldt, const double *Xs, long M, long Mpad,
                    const double *X, long N, long Npad, const KernParams &kp, int nb = 1, long sT = 0, long sX = 0,
                    const KernParams *kpt = nullptr);

// the same for M <= 8 candidate rows only (rows 0 .. M-1 of T, columns 0 .. Npad-1; no padding rows): the small-M path
void launch_cross_k_rows(hipStream_t s, double *T, long ldt, const double *Xs, int M, const double *X, long N, long Npad,
                         const KernParams &kp);

// logdet = 2 * sum_i log A[i*lda+i], i < N (deterministic single-block reduction)
void launch_logdet(hipStream_t s, const double *A, long lda, long N, double *out, int nb = 1, long sA = 0, long so = 0);
// out[p] = sum_i z_p[i]^2 for the RHS rows z_p = A[(Npad+p)*lda + i]
void launch_rhs_sumsq(hipStream_t s, const double *A, long lda, long N, long Npad, int P, double *out);

// Backward substitution alpha = L^-T z using the inverse diagonal tiles.
//   z rows: Z + p*ldz (p < P), alpha rows: Aout + p*ldz; w: workspace P*Npad; invP: inverted diagonal panels.
void launch_trsv_backward(hipStream_t s, const double *L, long lda, const double *invP, int W, long Npad, const double *Z, long ldz,
                          int P, double *Aout, double *w, int nb = 1, long sL = 0, long sP = 0, long sV = 0);

// Row reductions over the solved candidate rows T[c, 0:N]:
//   var[c] = kss - sum_i T[c,i]^2 (+ noise_add), mean[c*P+p] = sum_i T[c,i] * Z[p*ldz + i]
void launch_predict_reduce(hipStream_t s, const double *T, long ldt, long M, long N, const double *Z,
                           long ldz, int P, double kss, double noise_add, double *mean, double *var);

// mu[i] = sum_j k(x_i, x_j) alpha[j]  (posterior mean at the training inputs, K generated on the fly)
void launch_train_mean(hipStream_t s, const double *X, long N, const KernParams &kp, const double *alpha,
                       double *mu);
// the same vector as y - d alpha (d = total diagonal added to K), O(N)
void launch_train_mean_identity(hipStream_t s, const double *Y, const double *alpha, double d, long N, double *mu);
// deterministic min / argbest reductions
void launch_min(hipStream_t s, const double *v, long n, double *out);

// acquisition values (negated) from mean/var; optional argbest
void launch_acq(hipStream_t s, int type, double par, double fmin, double y_mean, double y_std,
                const double *mean, const double *var, long M, double *out);
void launch_argbest(hipStream_t s, const double *v, long n, int sense, double *best_val, long long *best_idx,
                    double *scratch_val, long long *scratch_idx);

// ---- mes.hip: max-value entropy search -- the rule over a table, and the sums the sampler of the minimum's value needs ---------
// the negated MES scores of M rows from their posterior (and, with dout, the x-gradients [M, D]): mes_terms of acq_math.h
void launch_mes_acq(hipStream_t s, const double *ystar, int K, double y_mean, double y_std, const double *mean, const double *var,
                    const double *dmdx, const double *dvdx, long M, int D, double *out, double *dout);
#define MES_CHUNK 256        // rows per chunk of the two-level sums (one workgroup, one row per thread)
#define MES_MAX_G 64         // trial values per launch (GP_MES_MAX_G)
struct MesY {
    int G;
    double y[MES_MAX_G];      // the trial values, by value
};
inline long mes_chunks(long M) { return (M + MES_CHUNK - 1) / MES_CHUNK; }
inline size_t mes_part_elems(long M) { return (size_t)(mes_chunks(M) + 1) * MES_MAX_G; }   // the chunks' sums, then the results
// res[g] = sum_{i < M} log Phi((m_i - y_g) / s_i): chunks of MES_CHUNK rows in row order, a fixed tree inside the chunk, the
// chunks in order; part: mes_part_elems(M) doubles, the results in its last MES_MAX_G
void launch_mes_logsurv(hipStream_t s, const double *mean, const double *var, long M, double y_mean, double y_std, const MesY &y,
                        double *part);
// res[0] = min_i (m_i - nsig s_i), res[1] = min_i (m_i + nsig s_i); part as above
void launch_mes_bracket(hipStream_t s, const double *mean, const double *var, long M, double y_mean, double y_std, double nsig,
                        double *part);

// ---- es.hip: entropy search -- the EP sweeps of p_min (one workgroup per chain) and the scoring of candidate rows -----------
void launch_es_pmin(hipStream_t s, const double *mu, const double *cov, int R, int max_sweeps, double tol, double *P, double *MP,
                    double *logS, int *status, int *sweeps);
// C [mc, ldc] latent covariance candidate x representer, var [mc] latent variance without noise; Qt [R, R, R] and Gt [R, R] with
// the belief index last; out [mc] the negated information gain
void launch_es_score(hipStream_t s, const double *C, long ldc, const double *var, long mc, double y_std, int R, const double *Qt,
                     const double *Gt, const double *logP, const double *u, const double *W, int S, double *out);

// ---- smallm.hip: a handful of candidate rows as matrix-vector work (the acquisition optimiser's one-row calls) ----------
// S[m, :] = T[m, :] L^-T for m < M by forward substitution over the panels (T consumed), inverted diagonal panels invP (W tiles)
void launch_small_forward_solve(hipStream_t s, const double *L, long lda, const double *invP, int W, long Npad, double *T,
                                double *S, long ldt, int M);
// beta[m, :] = Kx[m, :] Wi for m < M (Wi symmetric, Npad x Npad)
void launch_small_wi_product(hipStream_t s, const double *Wi, long ldw, long Npad, const double *Kx, long ldk, int M,
                             double *beta, long ldb);

// ---- onerow.hip: the acquisition optimiser's one-row calls as three launches over the explicit inverse factor ------------------
#define ROWS_MAX_M 4       // locations per pass of the fused path
#define ROWS_WIDE_M 8      // ... or per WIDE pass: 5 .. 8 locations in one read of the inverse factor (option "rows_wide")
#define ROWS_MAX_XS 128    // ... with M * D <= ROWS_MAX_XS doubles travelling in the kernel arguments
struct RowsX {
    int M;
    double xs[ROWS_MAX_XS];   // [M][D] row-major, as the caller gave them
};
struct RowsAcq {
    int on;                   // 0: posterior only
    int type;                 // GP_ACQ_*
    double par, fmin, y_mean, y_std;
    int lp, transform, nb;    // local penalisation (LP.py): on / log transform / batch size
    const double *Xb, *r0, *s0;
    const double *mes_y;      // GP_ACQ_MES: the K samples of the minimum's value on the device (the MES instances of the finish read them)
    int mes_K;
};
struct RowsMean {             // the affine mean function of a P = 1 model (mean.hip): A [D] and b [1] on the device; on = 0: none
    int on;
    const double *A, *b;
};
#define ROWS_OUT_DOUBLES (3 * ROWS_WIDE_M * (1 + GP_MAX_D))   // result block (sized for a wide pass); one more double behind it carries the call's ticket
struct RowsWork {             // device scratch (api_rows.hip sizes it): every partial has one writer
    double *wpart, *bpart, *meanpart, *vpart, *gpart;
};
// Where a pass reports (host side: the launchers of the three fused rows paths unpack it into the LAST arguments of their
// finishing kernel, in this order; the ensemble alone has the second base).  The path's PassOwner (api_internal.h) hands out
// one per pass and checks the ticket after the sync.
struct PassReport {
    unsigned int *counter;    // arrival counter of the finishing kernels: never reset between calls, each pass counts from its own base
    unsigned int base, base2; // ... the ensemble's two: of member z's workgroups at counter[1 + z], of the members at counter[0]
    double *out;              // pinned, host-visible result block
    double ticket;            // written behind the results by the workgroup that finishes the pass: the host checks it (a launch that
                              // did not complete must not leave the previous call's numbers in the block)
};
inline int rows_layout(int M) { return M == 1 ? 1 : M <= ROWS_MAX_M ? ROWS_MAX_M : ROWS_WIDE_M; }   // the MV a pass of M locations is laid out for
long rows_tiles(int nt);
int rows_block_height(int nt);   // rows of the tile per workgroup: 32 for matrices of a few tiles, else 128
size_t rows_gpart_elems(long N);
// Workgroups of the pass's last launch -- the arrivals its counter waits for; the host adds the same number to the counter's base
// after every pass (PassOwner::wait, api_internal.h), so launcher and host take it from here.
inline unsigned rows_finish_grid(long N) { return (unsigned)((N + 63) / 64); }       // rows_finish_kernel: 64 training rows per workgroup
inline unsigned rows_mean_grad_grid(long N) { return (unsigned)((N + 255) / 256); }  // rows_mean_grad_kernel: one row per thread
// results (host-visible block of 3 MV (1 + D) doubles, MV = rows_layout(M): 1 for M = 1, ROWS_MAX_M up to 4, ROWS_WIDE_M above):
//   [mean MV][var MV][acq MV][dmdx MV D][dvdx MV D][dacq MV D]
void launch_rows(hipStream_t s, const double *Li, long Npad, const RowsX &rx, const KernParams &kp, const double *X, long N,
                 const double *alpha, int want_grad, double kss, double noise_add, const RowsAcq &aq, const RowsWork &w,
                 const PassReport &r, int nt_loads, const RowsMean &mf = RowsMean{0, nullptr, nullptr});
// (mf.on: the mean-bearing instances of the finishing kernel add m(x) to the mean and A to dmdx; off: the instances and bits as ever)
// the forward launch of launch_rows alone: w.wpart (and w.meanpart) of the pass, no finishing kernel, no arrival at the counter
void launch_rows_forward(hipStream_t s, const double *Li, long Npad, const RowsX &rx, const KernParams &kp, const double *X, long N,
                         const double *alpha, const RowsWork &w, int nt_loads);
// the backward launch alone, behind launch_rows_forward of M locations: w.bpart and w.vpart from w.wpart
void launch_rows_backward(hipStream_t s, const double *Li, long Npad, int M, const RowsWork &w, int nt_loads);
// the mean's gradient alone: dmdx [M, D] at r.out + 3 MV (one pass over the training points, no inverse factor)
void launch_rows_mean_grad(hipStream_t s, const RowsX &rx, const KernParams &kp, const double *X, long N, const double *alpha,
                           const RowsWork &w, const PassReport &r, const RowsMean &mf = RowsMean{0, nullptr, nullptr});
// es.hip: a handful of locations behind the fused rows path's forward pass (launch_rows_forward): the scores into r.out at the
// acquisition's place of the rows layout, the ticket behind them; cpart: es_rows_part_elems(Npad) doubles; es_rows_grid(Npad)
// workgroups arrive at the pass's counter
unsigned es_rows_grid(long Npad);
size_t es_rows_part_elems(long Npad);
void launch_es_rows(hipStream_t s, const RowsX &rx, const KernParams &kp, const double *Xr, int R, const double *VR, long Npad,
                    const double *wpart, double *cpart, double kss, double y_std, const double *Qt, const double *Gt,
                    const double *logP, const double *u, const double *W, int S, const PassReport &r);
void launch_transpose_tri(hipStream_t s, double *dst, const double *src, long n, int mode);

// ---- paths.hip: posterior function samples by pathwise conditioning (api_paths.hip) --------------------------------------------
// f_s(x) = amp sum_j Wt[s, j] cos(omega_j . x + phase_j) + sum_n k(x, X_n) V[s, n].  omega [Fpad, D], phase [Fpad], Wt [Spad, Fpad],
// V [Spad, ldv]: Spad and Fpad multiples of PATHS_MMA, zeros in the padding
#define PATHS_MMA 16           // rows / columns of the fp64 matrix instruction: the padding of S and F
#define PATHS_MAX_SPAD 64      // GP_PATHS_MAX_S rounded up to it
#define PATHS_ROWS_M 8         // locations per launch_paths_rows (GP_PATHS_MAX_ROWS)
#define PATHS_ROWS_CH 256      // training rows / features per first-level partial of launch_paths_rows
#define PATHS_ROWS_GROW (ROWS_MAX_XS + PATHS_ROWS_M)   // doubles of per-workgroup sums: value and D gradient entries per location
struct PathsPrior {
    int F, Fpad, Spad;
    double amp;
    const double *omega, *phase, *Wt;
};
// R[s, n] = Y[n] - amp sum_j Wt[s, j] cos(omega_j . X_n + phase_j) - sd R[s, n] for s < S, n < N (R holds z_eps on entry); R [., ldr]
void launch_paths_residual(hipStream_t s, const PathsPrior &pp, int S, int D, const double *X, const double *Y, long N, double sd,
                           double *R, long ldr);
// out[s, i] = y_std f_s(xs_i) + y_mean for s < S, i < M: out [S, M]; part: paths_table_part_elems(M, N, S) doubles of scratch (0: a
// table of so many rows that one workgroup per 64 of them fills the chip; part may then be null)
size_t paths_table_part_elems(long M, long N, int S);
size_t paths_table_lds_bytes(int D, int Spad);   // LDS bytes a workgroup of that launch needs
void launch_paths_table(hipStream_t s, const PathsPrior &pp, int S, const KernParams &kp, const double *Xs, long M, const double *X,
                        long N, const double *V, long ldv, double y_mean, double y_std, double *out, double *part);
// per path s < S the best of tab[s, 0 .. M) (lowest index among ties) into rv[s] / ri[s]; rv / ri hold paths_argbest_elems(S)
// entries each: the results, then the first-level winners
inline long paths_argbest_elems(int S) { return (long)S * 257; }
void launch_paths_argbest(hipStream_t s, const double *tab, long M, int S, int sense, double *rv, long long *ri);
// rx.M <= PATHS_ROWS_M locations by value, location m on path `path[m]`: value at r.out[m], gradient (want_grad) at
// r.out[PATHS_ROWS_M + m D + d], the ticket at r.out[ROWS_OUT_DOUBLES]; gpart: paths_rows_grid(N, F) PATHS_ROWS_GROW doubles
struct PathsPick { int path[PATHS_ROWS_M]; };
inline unsigned paths_rows_grid(long N, int F) { return (unsigned)((N + PATHS_ROWS_CH - 1) / PATHS_ROWS_CH + (F + PATHS_ROWS_CH - 1) / PATHS_ROWS_CH); }
void launch_paths_rows(hipStream_t s, const PathsPrior &pp, const RowsX &rx, const PathsPick &pk, const KernParams &kp, const double *X,
                       long N, const double *V, long ldv, int want_grad, double y_mean, double y_std, double *gpart,
                       const PassReport &r);

// ---- qei.hip: the joint expected improvement of q <= ROWS_WIDE_M locations behind the fused rows path's passes (api_qei.hip) ------------
// result block (r.out): [value][status][mean q][cov q x q, row-major][dout q x D]; the ticket at r.out[ROWS_OUT_DOUBLES]
#define QEI_MAX_S 4096
#define QEI_OUT_VALUE 0
#define QEI_OUT_STATUS 1
#define QEI_OUT_MEAN 2
#define QEI_OUT_COV (QEI_OUT_MEAN + ROWS_WIDE_M)
#define QEI_OUT_GRAD (QEI_OUT_COV + ROWS_WIDE_M * ROWS_WIDE_M)
// state (device, QEI_STATE_DOUBLES): what the joint step leaves the closing pass: [status][mbar q][A q x q], both for the NORMALISED model
#define QEI_STATE_DOUBLES (1 + ROWS_WIDE_M + ROWS_WIDE_M * ROWS_WIDE_M)
struct QeiArgs {
    const double *Z;          // base samples on the device, COLUMN-major: entry (s, l) at Z[l * ldz + s]; a call of q locations reads
    int S, ldz;               // the leading q columns
    double par, fmin, y_mean, y_std;
};
// w_i . w_j for j <= i < M from w.wpart (laid out for rows_layout(M)): per 64 training rows one partial at w.gpart, in the order of
// the finishing kernel's value call
void launch_qei_gram(hipStream_t s, int M, long N, long Npad, const RowsWork &w);
// one workgroup: m, Sigma, its factor, the samples, the adjoint; value / mean / cov into r.out, mbar and A into state.  A pivot that
// is not positive or not finite: its 1-based row into both status words and nothing else.  want_grad = 0: the ticket as well.
void launch_qei_joint(hipStream_t s, const RowsX &rx, const KernParams &kp, long N, long Npad, const RowsWork &w, double kss,
                      double noise_add, const QeiArgs &qa, int want_grad, double *state, const PassReport &r);
// the closing pass over the training points: rows_finish_grid(N) workgroups arrive at the pass's counter, the last one writes the
// negated gradient [M, D] at r.out + QEI_OUT_GRAD (status 0) and the ticket (always)
void launch_qei_close(hipStream_t s, const RowsX &rx, const KernParams &kp, const double *X, long N, long Npad, const double *alpha,
                      const RowsWork &w, const double *state, const PassReport &r);

// ---- kg.hip: the discrete knowledge gradient over A resident discretisation points (api_kg.hip) -----------------------------------------
// C [mc, ldc] latent covariance candidate x point, mean / var [mc] the candidates' latent posterior (var without noise), muA [A] the
// points' latent means; out [mc] = +KG
void launch_kg_score(hipStream_t s, const double *C, long ldc, const double *mean, const double *var, long mc, double y_std,
                     double noise, int A, const double *muA, double *out);
// state (device): per location KG_STATE_STRIDE doubles [cv_i, i < A | ... | cw at 256 | cm at 257], what the scoring leaves the mix and
// the closing pass (kg.hip)
#define KG_STATE_STRIDE 264
// behind launch_rows_forward (two launches: the shares, then one workgroup per location): -KG into r.out at the acquisition's place
// of the rows layout; rx.M workgroups arrive at the pass's counter from r.base; cpart: kg_rows_part_elems(Npad) doubles.
// want_grad = 0: the ticket as well; else the state rows.
unsigned kg_rows_grid(long Npad);
size_t kg_rows_part_elems(long Npad);
void launch_kg_rows(hipStream_t s, const RowsX &rx, const KernParams &kp, const double *Xa, int A, const double *VA, const double *muA,
                    long Npad, const RowsWork &w, double *cpart, double kss, double noise, double y_std, int want_grad, double *state,
                    const PassReport &r);
// w.wpart <- the adjoint's right-hand sides cw_m w_m + sum_i cv_mi V_A[i] (chunk 0; zeros in the other chunks), for launch_rows_backward
void launch_kg_mix(hipStream_t s, int M, long N, long Npad, const RowsWork &w, const double *VA, int A, const double *state);
// the closing pass over the training points: rows_finish_grid(N) workgroups arrive at the pass's counter from counter_base, the last
// one writes the negated gradient [M, D] at the rows layout's dacq and the ticket
void launch_kg_close(hipStream_t s, const RowsX &rx, const KernParams &kp, const double *X, long N, long Npad, const double *alpha,
                     const RowsWork &w, const double *Xa, int A, const double *state, const PassReport &r, unsigned counter_base);

// ---- nei.hip: noisy expected improvement over S <= NEI_SPAD fantasies of the training values (api_nei.hip) ----------------------------
#define NEI_SPAD 64            // GP_NEI_MAX_S: rows of the fantasy-major blocks A0, U, F (zero rows beyond S)
// G[s ldg + i] = sum_{j <= i} L[i ldl + j] Zt[j NEI_SPAD + s], i < N, s < NEI_SPAD: one read of L's lower triangle.  Zt [N, NEI_SPAD]
// holds the draws transposed, zero columns beyond S.  Each (s, i) is its own dot product in j order
void launch_nei_lz(hipStream_t s, const double *L, long ldl, long N, const double *Zt, double *G, long ldg);
// mode 0: B[s, i] = y_i - sd Em[s, i] (into F) and R[s, i] = B[s, i] - G[s, i] (G holds g on entry, the residual on exit);
// mode 1: F[s, i] = F[s, i] - dd V[s, i].  s < S, i < N; every block fantasy-major [., ld], Em (the draws E) included
void launch_nei_assemble(hipStream_t s, int mode, int S, long N, const double *Y, const double *Em, double sd, double dd, double *G,
                         const double *V, double *F, long ld);
// fstar[s] = min_i F[s ld + i], i < N: one workgroup per fantasy, a fixed tree, no atomics
void launch_nei_colmin(hipStream_t s, const double *F, long ld, long N, int S, double *fstar);
// the X of two handles compared on the device: flag[0] = 1 where an entry differs (flag zeroed by the caller on the stream)
void launch_nei_same_x(hipStream_t s, const double *Xa, const double *Xb, long n, int *flag);
// table: mtab [S, M] = sum_n k(x_i, X_n) A0[s, n] (normalised), var [M] the twin's predictive variance with noise; out [M] = +NEI
void launch_nei_score(hipStream_t s, const double *mtab, const double *var, long M, int S, const double *fstar, double par,
                      double y_mean, double y_std, double *out);
// state (device): per location KG_STATE_STRIDE doubles laid out as the knowledge gradient's, [cv_s = -y_std p_s, s < S | ... |
// cw = -c y_std^2 / sd at 256 (0 where the floor holds) | cm = 0 at 257]: launch_kg_mix and launch_kg_close serve the gradient
// with U in V_A's place and no cross terms (A = 0 in the closing pass).
// behind launch_rows_forward (two launches: the shares, then one workgroup per location): -NEI into r.out at the acquisition's
// place of the rows layout; rx.M workgroups arrive at the pass's counter from r.base; cpart: nei_rows_part_elems(Npad) doubles.
// want_grad = 0: the ticket as well; else the state rows.  Returns the kernels it launched (2)
unsigned nei_rows_grid(long Npad);
size_t nei_rows_part_elems(long Npad);
int launch_nei_rows(hipStream_t s, const RowsX &rx, const KernParams &kp, const double *X, long N, long Npad, const double *A0, int S,
                     const double *fstar, const RowsWork &w, double *cpart, double kss, double noise_add, double par, double y_mean,
                     double y_std, int want_grad, double *state, const PassReport &r);

// ---- ens_rows.hip: the same passes over an ensemble of S members, the member as a grid dimension --------------------------------
#define ENS_ROWS_RB 32                       // rows of the tile per workgroup: what rows_block_height gives every matrix the ensemble takes
#define ENS_POST_STRIDE ROWS_OUT_DOUBLES     // doubles between two members' result blocks (each laid out as the single model's)
struct EnsRows {              // member z's operand at base + z * stride
    const double *Li;         // inverse factors, Npad x Npad each
    long sLi;
    const double *alpha;
    long sAlpha;
    const KernParams *kpt;    // per-member parameters
    const double *noise, *fmin;
    double *wpart, *bpart, *meanpart, *vpart, *gpart;   // RowsWork partials per member
    long sW, sB, sM, sV, sG;
    double *post;             // per-member result blocks
    unsigned int *counter;    // [0]: members arrived; [1 + z]: workgroups of member z arrived (neither is ever reset between passes)
};
// One pass of rx.M <= ROWS_MAX_M locations: forward (+ backward) + finish, whatever S.  Member z's workgroups count from r.base
// at counter[1 + z], the members from r.base2 at counter[0]; the host adds rows_finish_grid(N) and S to them after the pass
// (PassOwner::wait).  acq_on: the integrated rule (type, par; negated) into the host-visible block r.out; the ticket lands behind
// it either way.  (t.counter is the owner's counter, as r.counter.)
void launch_ens_rows(hipStream_t s, const EnsRows &t, int S, const RowsX &rx, const double *X, long N, long Npad, int want_grad,
                     int include_noise, int acq_on, int type, double par, const PassReport &r);
// out[c] = mean over members of the negated rule at candidate row c < M, from Kx = K_z(Xs, X) and W = Kx Li_z^T ([S][ldr][Npad] each)
void launch_ens_table_reduce(hipStream_t s, const double *Kx, const double *W, long ldr, long Npad, long N, const double *alpha,
                             long sAlpha, const KernParams *kpt, const double *noise, const double *fmin, int S, int type, double par,
                             long M, double *out);

// ---- append.hip: a border of k <= 128 new rows inside one diagonal tile (gp_append) ------------------------------------------------
#define GP_APPEND_V 8      // new rows per pass over the factor / the inverse factor
// O[c ldo + i] = sum_{j <= i} Mat[i ld + j] V[c ldv + j], i < n, c < kc <= GP_APPEND_V: Mat lower triangular (zeros above the diagonal),
// ncols allocated columns (even), V finite up to ncols.  Rows n .. of O are left alone.
void launch_append_rowdot(hipStream_t s, const double *Mat, long ld, long n, long ncols, const double *V, long ldv, int kc, double *O,
                          long ldo, int nt_loads);
// R[c ldr + j] = sum_{i >= j, i < n} V[c ldv + i] Mat[i ld + j] for j < n, 0 for n <= j < ncols, c < kc <= GP_APPEND_V, through the
// partials part: append_col_chunks(n) GP_APPEND_V ldp doubles with ldp >= n rounded up to GP_TILE
int append_col_chunks(long n);
void launch_append_colsum(hipStream_t s, const double *Mat, long ld, long n, long ncols, const double *V, long ldv, int kc, double *part,
                          long ldp, double *R, long ldr, int nt_loads);
// S (one tile, symmetric, the identity beyond k) = Knn + ((Euclidean: variance, Gower: Knn's own diagonal) + diag_add + jitter) I -
// T T^T for the k rows T of n entries; gpart: append_gram_elems(n, k) doubles; flag[0] = 1 where an entry of S is not finite
long append_gram_elems(long n, int k);
void launch_append_schur(hipStream_t s, const double *T, long ldt, long n, int k, double *gpart, const double *Knn, double variance,
                         int gower, double diag_add, double jitter, double *S, int *flag);
// O[a ldo + j] = -sum_{b <= a} Linv[a 128 + b] R[b ldr + j], a < k, j < ncols
void launch_append_negmul(hipStream_t s, const double *Linv, const double *R, long ldr, int k, long ncols, double *O, long ldo);
// rows row0 .. row0 + k - 1 of dst = [ src21 (columns < c0) | lower triangle of the tile tile22 | 0 ] over ncols columns
void launch_append_commit_rows(hipStream_t s, double *dst, long ld, long ncols, long row0, int k, long c0, const double *src21, long ld21,
                               const double *tile22);
void launch_append_identity_rows(hipStream_t s, double *dst, long ld, long ncols, long r0, long r1);
// O[p ldo + i] = Y[i P + p], i < N; 0 for N <= i < ncols
void launch_append_yrows(hipStream_t s, const double *Y, long N, int P, long ncols, double *O, long ldo);

// ---- grad.hip ---------------------------------------------------------------------------------
#define GP_GRAD_CH 16
#define GP_GRAD_NACC (GP_GRAD_CH + 2)
void launch_set_identity(hipStream_t s, double *T, long ld, long n);
void launch_symmetrize(hipStream_t s, double *A, long ld, long n, int nb = 1, long sA = 0);
// A = scale * lower(A), mirrored into the upper triangle
void launch_symmetrize_scale(hipStream_t s, double *A, long ld, long n, double scale, int nb = 1, long sA = 0);
// LDS bytes a workgroup of that launch needs, its static part included, from (kp.D, kp.gower, P)
size_t lml_grad_lds_bytes(int D, int gower, int P);
void launch_lml_grad(hipStream_t s, const double *X, long N, long Npad, const KernParams &kp, int ard, int d0, const double *alpha,
                     int P, const double *Wi, long ldw, double *partial, double *out, int nb = 1, const KernParams *kpt = nullptr,
                     long sV = 0, long sW = 0, long sP = 0, long so = 0, long sX = 0);
// the same pass with the weights of the Laplace marginal, dL_dK = 1/2 (a a^T + a u^T + u a^T - R): au [2, Npad] holds a and u,
// R [Npad, ldr] = (K + W^-1)^-1; one member, no Gower model.  LDS: lml_grad_lds_bytes(D, 0, 2)
void launch_lap_grad(hipStream_t s, const double *X, long N, long Npad, const KernParams &kp, int ard, int d0, const double *au,
                     const double *R, long ldr, double *partial, double *out);

// ---- laplace.hip: GP classification, Laplace's method with a probit link (api_laplace.hip) -----------------------------------
// labels y in {-1, +1}; every vector has Npad entries; K is the full Npad x Npad matrix of launch_kbuild(full = 1, diag_add = 0)
void launch_lap_site(hipStream_t s, const double *y, const double *f, long N, long Npad, double *W, double *sw, double *b, double *t);
// out_i = scale_i sum_j M[i, j] v_j (scale null: 1), or from_i - that; i, j < N
void launch_lap_matvec(hipStream_t s, const double *M, long ld, const double *v, long N, const double *scale, const double *from,
                       double *out);
void launch_lap_bbuild(hipStream_t s, double *A, long lda, const double *K, long ldk, const double *sw, long N, long Npad);
void launch_lap_dir(hipStream_t s, const double *b, const double *sw, const double *w, const double *a, long N, long Npad, double *da);
#define LAP_RES_DOUBLES 8   // res of launch_lap_psi: psi, -a.f / 2, sum log p, max |da|, max |a + step da|; of launch_lap_wrange: min, max
void launch_lap_psi(hipStream_t s, const double *y, const double *a, const double *da, const double *f, const double *df, double step,
                    long N, double *res);
void launch_lap_accept(hipStream_t s, double *a, const double *da, double *f, const double *df, double step, long N);
void launch_lap_wrange(hipStream_t s, const double *W, long N, double *res);
void launch_lap_scale_factor(hipStream_t s, double *A, long lda, double *invL, const double *sw, long N, long Npad);
void launch_lap_ltvec(hipStream_t s, const double *A, long lda, const double *a, long N, long Npad, double *z);
void launch_lap_s2(hipStream_t s, const double *R, long ldr, const double *W, const double *t, long N, long Npad, double *s2);
void launch_predict_grad(hipStream_t s, const double *Xs, long M, const double *X, long N, const KernParams &kp,
                         const double *alpha, long lda_, int P, const double *beta, long ldb, double *dmdx,
                         double *dvdx);
void launch_acq_grad(hipStream_t s, int type, double par, double fmin, double y_mean, double y_std, const double *mean,
                     const double *var, const double *dmdx, const double *dvdx, long M, int D, double *out,
                     double *dout);
void launch_add_diag(hipStream_t s, double *A, long lda, long N, double v, int nb = 1, long sA = 0, const double *v_tab = nullptr);
void launch_trace(hipStream_t s, const double *A, long lda, long N, double *out);   // out[0] = trace, out[1] = smallest diagonal entry

// nb blocks of n x n (row-major, leading dimension n, stacked): identity / transpose (dst_b = src_b^T)
void launch_set_identity_blocks(hipStream_t s, double *T, long n, int nb);
void launch_transpose_blocks(hipStream_t s, double *dst, const double *src, long n, int nb);
void launch_lp(hipStream_t s, const double *negacq, const double *Xs, long M, int D, const double *Xb, int nb,
               const double *r0, const double *s0, int transform, double *out);
void launch_lp_grad(hipStream_t s, double *negacq, double *dneg, const double *Xs, long M, int D, const double *Xb, int nb,
                    const double *r0, const double *s0, int transform);
void launch_mask(hipStream_t s, double *v, const long long *idx, int n, double fill);
// out[i, j] = 0.5 (sum_p alpha_p[i] alpha_p[j] - P Wi[i, j]),  i, j < N  (exact_gaussian_inference.py:70)
void launch_dldk(hipStream_t s, double *out, long ldo, const double *alpha, long lda_, int P, const double *Wi,
                 long ldw, long N);
// zero the strict upper triangle of the nt diagonal 128-tiles (the factor's tiles keep the symmetric input there)
void launch_zero_upper_diag(hipStream_t s, double *A, long lda, int nt);

// ---- gradx.hip: input-side kernels of the input-warped GP -------------------------------------------------------------
// out[i, q] = dL/dX_iq for i < N (row-major [N, D]): sum_j 2 dL_dK_ij g(r_ij) (x_iq - x_jq) / l_q^2 with dL_dK = 0.5 (alpha alpha^T -
// P Wi), one pass over Wi (both triangles) per GP_GRAD_CH dimensions; partial: gradx_partial_elems(Npad) doubles of scratch
long gradx_partial_elems(long Npad);
size_t gradx_lds_bytes(int D, int P);   // LDS bytes a workgroup of launch_gradx needs
// (nb members: member z's inputs at X + z sX, rows at out + z so, the rest as launch_lml_grad)
void launch_gradx(hipStream_t s, const double *X, long N, long Npad, const KernParams &kp, const double *alpha, int P,
                  const double *Wi, long ldw, double *partial, double *out, int nb = 1, const KernParams *kpt = nullptr,
                  long sX = 0, long sV = 0, long sW = 0, long sP = 0, long so = 0);
// rows [m0, m0 + mc) of the resident [M, D] table Xs (m0 D even) through the Kumaraswamy CDF, in place, where warp[q] is set
void launch_kumar_warp(hipStream_t s, double *Xs, long m0, long mc, int D, const int *warp, const double *a, const double *b,
                       const double *xmin, const double *xmax);

// ---- sparse.hip: kernels of the sparse GP (variational DTC) -------------------------------------------------------------------
#define GP_SPARSE_GRAD_MAX_P 16               // outputs whose woodbury-vector row stays in the gradient lane's registers
#define GP_SPARSE_NH (1 + GP_GRAD_CH)         // hyper-parameter sums per pass of GP_GRAD_CH dimensions: sum W k, then sum W g d_q^2
// One pass per GP_GRAD_CH dimensions over the Nc x Mz block of weights W[n, m] = wscale Wt[n ldw + m] + ybeta sum_p Y[n, p] C[p ldc + m]
// (P = 0: no y term) between the rows Z [Mz, D] and the columns Xc [Nc, D]:
//   dZ[m, q]                  = zfac / l_q sum_n W g(r) d_q,   d_q = (z_mq - x_nq) / l_q
//   hyper[pass GP_SPARSE_NH]     = sum_nm W k;   hyper[pass GP_SPARSE_NH + 1 + q] = sum_nm W g(r) d_q^2   (q = dimension - pass GP_GRAD_CH)
// partial: sparse_grad_partial_elems(Mzpad, Nc) doubles of scratch; Wt has at least Nc rows of ldw >= Mzpad entries
long sparse_grad_partial_elems(long Mzpad, long Nc);
size_t sparse_grad_lds_bytes(int D, int P);   // LDS bytes a workgroup of launch_sparse_grad needs
// mb (gp_sparse_fit_grad_batch): the same pass for mb->nb members in the same launches, member z = blockIdx.z with rows Z + z sZ,
// columns Xc + z sXc (0: shared), parameters kpt[z] (device; kp then only picks the instance and the LDS size), woodbury rows
// C + z sC, weights Wt + z sW, ybeta_tab[z] / wscale_tab[z] in place of ybeta / wscale (null: the value given), slabs at
// partial + z sP, results at dZ + z sDZ and hyper + z sH.  The chunking of the columns and the order of every sum are functions of
// (Nc, Mz) alone: a member gets the bits it gets alone.  Null: one problem, as before.
struct SparseGradMembers {
    int nb = 1;
    long sZ = 0, sXc = 0, sC = 0, sW = 0, sP = 0, sDZ = 0, sH = 0;
    const KernParams *kpt = nullptr;
    const double *ybeta_tab = nullptr, *wscale_tab = nullptr;
};
void launch_sparse_grad(hipStream_t s, const double *Z, long Mz, long Mzpad, const double *Xc, long Nc, const KernParams &kp,
                        const double *Y, int P, const double *C, long ldc, double ybeta, const double *Wt, long ldw, double wscale,
                        double *partial, double zfac, double *dZ, double *hyper, const SparseGradMembers *mb = nullptr);
// n x n helpers (leading dimension n): out = a X + b Y + c I (Y may be null);  out = c I + sum_p v_p v_p^T, v_p = V + p ldv.
// nb members per launch: member z's operands at base + z stride, a_tab[z] / b_tab[z] / scale_tab[z] in place of a / b / scale
// where a table is given.  The defaults are the single problem.
void launch_sparse_lincomb(hipStream_t s, double *out, const double *X, double a, const double *Y, double b, double c, long n, int nb = 1,
                           long sO = 0, long sX = 0, long sY = 0, const double *a_tab = nullptr, const double *b_tab = nullptr);
void launch_sparse_outer(hipStream_t s, double *out, const double *V, long ldv, int P, double c, long n, int nb = 1, long sO = 0,
                         long sV = 0);
// out[p ldo + i] = scale sum_{k < K} M[i ldm + k] v[p vsp + k vsk],  i < rows, p < P  (members: M + z sM, v + z sv, out + z so)
void launch_sparse_thin(hipStream_t s, const double *M, long ldm, long rows, long K, const double *v, long vsp, long vsk, int P,
                        double scale, double *out, long ldo, int nb = 1, long sM = 0, long sv = 0, long so = 0,
                        const double *scale_tab = nullptr);
// out[0] = sum Y^2 (NP entries), out[1] = trace VVt (Mz), out[2] = sum c1^2 (P rows of n), out[3] = sum VVt o Dm (n x n)
// (members: Y shared, VVt / Dm + z sT, c1 + z sc, out + z so)
void launch_sparse_scalars(hipStream_t s, const double *Y, long NP, const double *VVt, const double *Dm, long Mz, long n, const double *c1,
                           int P, double *out, int nb = 1, long sT = 0, long sc = 0, long so = 0);
// mean[c, p] = sum_m Kx[c, m] w[p ldw + m];  var[c] = max(kss - sum_m Bt[c, m] Kx[c, m], 1e-15) + noise_add,  c < M, m < Mz
void launch_sparse_predict_reduce(hipStream_t s, const double *Kx, const double *Bt, long ld, long M, long Mz, const double *w, long ldw,
                                  int P, double kss, double noise_add, double *mean, double *var);
void launch_sparse_min(hipStream_t s, const double *v, long n, double *out);

// ---- sparse_rows.hip: a handful of locations on the sparse model as ONE launch over woodbury_inv ------------------------------
#define SPARSE_ROWS_RB 8                                       // rows of woodbury_inv per workgroup (two per wave)
#define SPARSE_ROWS_GROW (2 * ROWS_MAX_XS + 2 * ROWS_WIDE_M)   // doubles of per-workgroup sums (gpart: grid rows of them)
// workgroups of a pass -- the arrivals its counter waits for (the host adds the same number to the counter's base after the pass:
// PassOwner::wait, api_internal.h)
inline unsigned sparse_rows_grid(long Mz) { return (unsigned)((Mz + SPARSE_ROWS_RB - 1) / SPARSE_ROWS_RB); }
// mode 0: mean / var (/ acquisition) of rx.M <= ROWS_WIDE_M locations with rx.M D <= ROWS_MAX_XS; 1: the gradients as well; 2: the
// mean's gradient alone (Winv not read).  Winv [n, n] with n = Mz rounded up to GP_TILE, Zs [Mz, D] = Z / lengthscale
// (launch_sparse_scale_z), w [Mz].  Results in the
// host-visible block r.out, laid out for ROWS_WIDE_M locations whatever rx.M: [mean][var][acq][dmdx D][dvdx D][dacq D], and
// the ticket at r.out[ROWS_OUT_DOUBLES].
void launch_sparse_scale_z(hipStream_t s, const double *Z, long Mz, const KernParams &kp, double *Zs);
void launch_sparse_rows(hipStream_t s, const double *Winv, long n, long Mz, const RowsX &rx, const KernParams &kp, const double *Zs,
                        const double *w, int mode, double kss, double noise_add, const RowsAcq &aq, double *gpart,
                        const PassReport &r);

// ---- sparse_cov.hip: the sparse posterior covariance between locations and a resident second point set --------------------------
#define SPARSE_COV_RB 8                                        // rows of G per workgroup (two per wave)
// workgroups along G's rows -- for the by-value launch the arrivals its counter waits for
inline unsigned sparse_cov_grid(long R) { return (unsigned)((R + SPARSE_COV_RB - 1) / SPARSE_COV_RB); }
// cov[i, r] = k(x1_i, x2_r) - sum_j G[r, j] k(x1_i, z_j) for r < R.  G [Rpad, n] = K(X2, Z) woodbury_inv (n = Mz rounded up to
// GP_TILE, Rpad = R rounded up to it, zero rows in the padding), X2s [R, D] and Zs [Mz, D] the points over the lengthscales
// (launch_sparse_scale_z).  _rows: the rx.M <= ROWS_WIDE_M locations of rx (rx.M D <= ROWS_MAX_XS) into the host-visible out
// [rx.M, R], the ticket at r.out[ROWS_OUT_DOUBLES].  _table: X1 [M1, D] and out [M1, R] on the device, in blocks of ROWS_WIDE_M
// locations through the same kernel body: a row has the same bits on either route, in any company.
void launch_sparse_cov_rows(hipStream_t s, const double *G, long n, long Mz, long R, const double *X2s, const RowsX &rx,
                            const KernParams &kp, const double *Zs, double *out, const PassReport &r);
void launch_sparse_cov_table(hipStream_t s, const double *G, long n, long Mz, long R, const double *X2s, const double *X1, long M1,
                             const KernParams &kp, const double *Zs, double *out);

// ---- cost.hip: the cost surface of cost-aware EI / MPI and the quotient it puts under the scores --------------------------------
// logc[i] = shift + scale sum_j alpha[j] k(xs_i, Xc_j) and (dlogc given) its x-gradient [M, D], over the surface Xcs = Xc / lengthscale
// [Nc, ld] (ld = max(D, 8), zeros beyond D).  One summation order per location in both launches: the same bits (cost.hip).
// part: cost_table_part_elems(M, Nc, D) doubles of scratch (0: none wanted) for a values-only call, which is then cut along the
// surface too -- a table of few rows on every compute unit; null: one workgroup per 64 / 256 candidates over the whole surface
size_t cost_table_part_elems(long M, long Nc, int D);
void launch_cost_table(hipStream_t s, const double *Xs, long M, const double *Xcs, int ld, const double *alpha, long Nc,
                       const KernParams &kp, double shift, double scale, double *logc, double *dlogc, double *part);
// rx.M <= ROWS_WIDE_M locations by value.  blk null: logc [M] (and, with grad, dlogc [M, D]) are written; blk given: the quotient is
// applied in place to the negated scores (and, with grad, their gradients) of a rows result block laid out for MV locations
void launch_cost_rows(hipStream_t s, const RowsX &rx, const double *Xcs, int ld, const double *alpha, long Nc, const KernParams &kp,
                      double shift, double scale, int grad, double *logc, double *dlogc, double *blk, int MV);
// neg <- neg / c, dneg <- (dneg - neg_old dlogc) / c with c = exp(logc), element-wise in place (dneg null: values only)
void launch_cost_apply(hipStream_t s, const double *logc, const double *dlogc, long M, int D, double *neg, double *dneg);

// ---- mean.hip: the affine mean function m(x) = x^T A + b of the exact GP ------------------------------------------------------------
// Ab: A [D, P] row-major, then b [P] (an absent part as zeros).  m(x)_p starts from b_p and takes the D products in dimension order
#define MEAN_GRAD_CH 256   // training rows per first-level partial of launch_mean_grad: the summation order's only constant
void launch_mean_residual(hipStream_t s, const double *X, const double *Y, long N, int D, int P, const double *Ab, double *R);   // R = Y - m(X)
void launch_mean_add(hipStream_t s, const double *Xs, long M, int D, int P, const double *Ab, double *mean);   // mean [M, P] += m(Xs)
void launch_mean_add_grad(hipStream_t s, long M, int D, int P, const double *Ab, double *dmdx);               // dmdx [M, D, P] += A
// out [(D + 1) P]: X^T alpha [D, P], then 1^T alpha [P]; alpha [P] rows of ldal; part: mean_grad_chunks(N) (D + 1) P doubles
int mean_grad_chunks(long N);
void launch_mean_grad(hipStream_t s, const double *X, const double *alpha, long ldal, long N, int D, int P, double *part, double *out);

// ---- feas.hip: the probability of feasibility of K constraint GPs and the product it puts behind EI / MPI ------------------------
// K constraints at a handful of locations: constraint k's normalised posterior -- mean / var [M], dm / dv [M, D] (read with grad
// only) on the device or in a pinned result block --, its output normaliser and its upper bound
#define FEAS_MAX_K 8   // constraints per call (GP_FEAS_MAX of the public header)
struct FeasRows {
    int K;
    const double *mean[FEAS_MAX_K], *var[FEAS_MAX_K], *dm[FEAS_MAX_K], *dv[FEAS_MAX_K];
    double bound[FEAS_MAX_K], c_mean[FEAS_MAX_K], c_std[FEAS_MAX_K];
};
// logF[i] = (first ? 0 : logF[i]) + log Phi((b - m_i) / s_i) over a table's posterior: the constraints are added one launch each
void launch_feas_table(hipStream_t s, const double *mean, const double *var, long M, double c_mean, double c_std, double b,
                       int first, double *logF);
// acq[i] <- (pof ? -1 : acq[i]) exp(logF[i])
void launch_feas_apply(hipStream_t s, const double *logF, long M, int pof, double *acq);
// M locations, one workgroup each.  neg given: neg [M] <- neg F and (grad) dneg [M, D] <- F (dneg + neg dlogF) in place, with pof
// neg = -1 and dneg = 0 taken as what came in; neg null: logF [M] and (grad) dlogF [M, D] are written.  The sum over k runs in
// index order, as launch_feas_table's launches do
void launch_feas_rows(hipStream_t s, const FeasRows &fr, int M, int D, int grad, int pof, double *neg, double *dneg, double *logF,
                      double *dlogF);
void launch_feas_gather(hipStream_t s, const double *v, const long long *rows, long n, double *out);   // out[i] = v[rows[i]]

// ---- ehvi.hip: expected hypervolume improvement of K independent objective GPs over a cell decomposition -------------------------
#define EHVI_MAX_K 3        // objectives (GP_EHVI_MAX_OBJ of the public header)
#define EHVI_MAX_L 256      // levels per objective (GP_EHVI_MAX_LEVELS)
#define EHVI_THREADS 256    // one workgroup of four waves per location
// The decomposition on the device: objective k's L[k] levels at levels + off[k] (entry 0 is -inf), and C cells of K words each,
// word [c * K + k] = lo | hi << 16 with lo < hi indices into objective k's levels
struct EhviCells {
    int K, C;
    int L[EHVI_MAX_K], off[EHVI_MAX_K];
    const double *levels;
    const unsigned int *cells;
};
// objective k's normalised posterior at the locations -- mean / var [M], dm / dv [M, D] (read with grad only), on the device or in
// a pinned result block -- and its output normaliser
struct EhviRows {
    const double *mean[EHVI_MAX_K], *var[EHVI_MAX_K], *dm[EHVI_MAX_K], *dv[EHVI_MAX_K];
    double y_mean[EHVI_MAX_K], y_std[EHVI_MAX_K];
};
// neg [M] <- -EHVI over a table's posteriors, one workgroup per row
void launch_ehvi_table(hipStream_t s, const EhviCells &ec, const EhviRows &er, long M, double *neg);
// M locations, one workgroup each: neg [M] <- -EHVI and (grad) dneg [M, D] <- -d EHVI / dx.  The same device routine as the table's
void launch_ehvi_rows(hipStream_t s, const EhviCells &ec, const EhviRows &er, int M, int D, int grad, double *neg, double *dneg);

// ---- rns.hip: fp64-equivalent contraction on the int8 matrix cores (option "emulate_fp64") -----------------------------
#define GP_RNS_T 14
#define GP_RNS_KMAX 8192   // longest contraction (bytes) one residue launch may take: see rns_reduce_f in rns.hip
int rns_init_constants(int device);
void launch_rns_convert(hipStream_t s, const double *src, long ld, long rows, long cols, signed char *dst,
                        long plane_stride, long ldd, double scale, int *flag);
void rns_set_interleave(int v);
void launch_rns_gemm256(hipStream_t s, const signed char *A, long lda, long a_plane, const signed char *B, long ldb,
                        long b_plane, signed char *R, int mt_all, int nt_all, int mt, int c0, int c1, int K,
                        int first, int tri = 0);
void launch_rns_reconstruct256(hipStream_t s, const signed char *R, int mt_all, int nt_all, int mt, int c0_128, int c1_128,
                               long rows, double *T, long ldt, double scale_2e, int tri = 0);
