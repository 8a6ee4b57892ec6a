// gp_fit_grad_batch: the LML and its hyper-parameter gradients for R parameter vectors over the context's (X, Y) in one call --
// the L-BFGS evaluations of R hyper-parameter restarts run in lockstep (GPRegression.optimize_restarts(parallel=True)).
// Reference: optimize_restarts over GPModel.updateModel (GPyOpt/GPyOpt/models/gpmodel.py:78-93), each evaluation being
// Model.objective_function + objective_function_gradients (GPy/GPy/core/model.py:96-127) of ExactGaussianInference
// (exact_gaussian_inference.py:37-74) with jitchol's ladder (linalg.py:56-81).
//
// Member r runs the launch sequence of gp_fit_grad's single-stream route -- fit_impl over factor_buf (128-column steps), the
// inverted diagonal panels of ensure_panel_inv, alpha / log det, the solve for L^-T and the k-panel product of wi_lauum, the
// fused gradient pass -- with the member as a batch index (blockIdx.z, or the GEMM's blockIdx.y) and per-member strides, so that
// R members cost the launches of ONE evaluation.  Every batched launch runs the body of its single-member kernel, and the GEMMs
// take the instance the single call picks for the same tile set: a member does the single call's per-tile arithmetic.
// The batch has buffers of its own: the context's resident fit (L, alpha, Ky^-1, parameters, fitted / predicted state) is left
// as it was.  Always true fp64 (option "emulate_fp64" does not apply).
#include "api_internal.h"

#define GP_BATCH_MAX_R 64
#define GP_BATCH_MAX_NPAD 2048

namespace {

// gemm() (api_core.hip) chooses the GEMM instance from the launch's tile count; a batch launch has R times the tiles of the
// single call, so the instance is chosen here from ONE member's tile set -- the instance the single call runs -- and the
// members ride on the kernel's batch index.
void bgemm(gp_ctx *g, int mode, double *C, long ldc, const double *A, long lda, const double *B, long ldb, int b_mul, int K,
           TileSet ts, GemmOpt o, int nb, long sC, long sA, long sB) {
    const long n = tileset_count(ts);
    if (n <= 0 || K <= 0 || nb <= 0) return;
    if (n >= 1024 && !o.stagger) o.stagger = g->stagger;
    if (n >= 1024 && g->waves8) o.waves8 = 1;
    if (o.inplace && g->trsm_rows64 && !o.waves8) o.rows64 = g->trsm_rows64;
    if (g->small_below > 0 && n < g->small_below && !o.inplace) o.small = 1;
    if (g->pair_tri && (o.small || (o.waves8 && g->pair_tri >= 2)) && o.k_end_tri && !ts.tri && ts.c1 - ts.c0 >= 2) o.pair = 1;
    o.batch = nb;
    o.sC = sC;
    o.sA = sA;
    o.sB = sB;
    launch_gemm_nt(g->s, mode, C, ldc, A, lda, B, ldb, b_mul, K, ts, o);
    g->gemm_flops_all += 2.0 * GP_TILE * GP_TILE * (double)K * (double)(n * nb) * ((o.k_tri || o.k_end_tri) ? 0.5 : 1.0);
}

// nb identity blocks of n x n, stacked: launch_set_identity_blocks in pieces whose grid stays within 32768 rows
void identity_blocks(hipStream_t s, double *T, long n, int nb) {
    const int per = (int)std::max(1L, 32768 / n);
    for (int b0 = 0; b0 < nb; b0 += per) launch_set_identity_blocks(s, T + (long)b0 * n * n, n, std::min(per, nb - b0));
}

struct BatchGeom {
    long N, Npad, lda;
    int nt, W, nJ, P;
    long PB;
    long sA, sI, sP, sV, sT, sS;   // per-member strides (doubles): factor + RHS rows, inverted tiles, inverted panels, alpha, N x N, scalars
};

// K build, jitter, RHS rows and the blocked Cholesky of factor_buf (no look-ahead, 128-column steps) for members [m0, m0 + nb)
void factor_members(gp_ctx *g, const BatchGeom &b, double *dA, double *dI, int *dInfo, const KernParams &kp0, const KernParams *kpt,
                    const double *diag, const double *jit, int m0, int nb, bool jittered) {
    const long lda = b.lda;
    double *A = dA + m0 * b.sA, *I = dI + m0 * b.sI;
    int *info = dInfo + m0 * 4;
    launch_kbuild_batch(g->s, A, lda, b.sA, g->dX, b.N, b.Npad, kp0, kpt + m0, diag + m0, nb);
    if (jittered) launch_add_diag_batch(g->s, A, b.sA, lda, b.N, jit + m0, nb);
    launch_set_rhs_batch(g->s, A, lda, b.sA, g->dY, b.N, b.Npad, b.P, nb);
    GP_NOTE(hipMemsetAsync(info, 0, sizeof(int) * 4 * nb, g->s));
    const int nt = b.nt, R1 = nt + 1, W = g->panel_tiles;
    for (int J0 = 0; J0 < nt; J0 += W) {
        const int J1 = std::min(J0 + W, nt);
        for (int j = J0; j < J1; ++j) {
            launch_potrf_tile_batch(g->s, A, lda, b.sA, j, I, b.sI, info, 4, nb);
            bgemm(g, 0, A, lda, A + (long)j * GP_TILE, lda, I + (long)j * GP_TILE * GP_TILE, GP_TILE, 0, GP_TILE,
                  TileSet{j + 1, R1, j, j + 1, 0}, inplace_opt(), nb, b.sA, b.sA, b.sI);
            if (j + 1 < J1)
                bgemm(g, 1, A, lda, A + (long)j * GP_TILE, lda, A + (long)j * GP_TILE, lda, 1, GP_TILE, TileSet{0, R1, j + 1, J1, 1},
                      GemmOpt(), nb, b.sA, b.sA, b.sA);
        }
        if (J1 < nt)
            bgemm(g, 1, A, lda, A + (long)J0 * GP_TILE, lda, A + (long)J0 * GP_TILE, lda, 1, (J1 - J0) * GP_TILE,
                  TileSet{0, R1, J1, nt, 1}, GemmOpt(), nb, b.sA, b.sA, b.sA);
    }
}

}  // namespace

extern "C" int gp_fit_grad_batch(gp_t *g, int R, const double *variance, const double *lengthscale, const double *noise, int maxtries,
                                 double *lml, double *logdet, double *jitter_used, double *dvariance, double *dlengthscale,
                                 double *dnoise, int *status) {
    if (!g || !variance || !lengthscale || !noise || !lml || !logdet || !jitter_used || !dvariance || !dlengthscale || !dnoise ||
        !status)
        return fail(GP_ERR_ARG, "null argument");
    GP_DEAD_CHECK(g);
    if (!g->have_data || !g->have_params) return fail(GP_ERR_STATE, "set data and params before gp_fit_grad_batch");
    if (R < 1) return fail(GP_ERR_ARG, "R must be at least 1");
    if (R > GP_BATCH_MAX_R) return fail(GP_ERR_ARG, "gp_fit_grad_batch takes at most R = %d members (got %d)", GP_BATCH_MAX_R, R);
    if (g->Npad > GP_BATCH_MAX_NPAD)
        return fail(GP_ERR_ARG, "gp_fit_grad_batch covers Npad <= %d (N = %ld pads to %ld): use gp_fit_grad", GP_BATCH_MAX_NPAD,
                    g->N, g->Npad);
    if (g->P > 16) return fail(GP_ERR_ARG, "gp_fit_grad_batch supports P <= 16");
    const int D = g->D, nls = g->ard ? D : 1;
    for (int r = 0; r < R; ++r) {
        if (!(variance[r] > 0.0)) return fail(GP_ERR_ARG, "member %d: variance must be positive", r);
        if (!(noise[r] > 0.0)) return fail(GP_ERR_ARG, "member %d: noise must be positive", r);
        for (int d = 0; d < nls; ++d)
            if (!(lengthscale[(long)r * nls + d] > 0.0)) return fail(GP_ERR_ARG, "member %d: lengthscale must be positive", r);
    }
    HIPCHK(hipSetDevice(g->device));

    BatchGeom b;
    b.N = g->N;
    b.Npad = g->Npad;
    b.lda = g->Npad;
    b.P = g->P;
    b.nt = (int)(b.Npad / GP_TILE);
    b.W = std::min(g->panel_tiles, b.nt);
    b.PB = (long)b.W * GP_TILE;
    b.nJ = (b.nt + b.W - 1) / b.W;
    b.sA = (b.Npad + GP_TILE) * b.Npad;
    b.sI = (long)b.nt * GP_TILE * GP_TILE;
    b.sP = (long)b.nJ * b.PB * b.PB;
    b.sV = (long)b.P * b.Npad;
    b.sT = b.Npad * b.Npad;
    b.sS = 64 + 4 * GP_GRAD_NACC;   // [0] log det, [8, 8 + P) alpha . y, [64 + pass * NACC ...) gradient sums (D <= 64: 4 passes)
    const long per = b.sA + b.sI + 2 * b.sP + 2 * b.sV + 2 * b.sT + b.sS + 2;
    int rc;
    if ((rc = dev_realloc(&g->dBatch, &g->capBatch, per * R))) return rc;
    const size_t kp_bytes = (sizeof(KernParams) * R + 255) / 256 * 256;
    if ((rc = byte_realloc(&g->dBatchAux, &g->capBatchAux, (long)(kp_bytes + sizeof(int) * 4 * R)))) return rc;
    double *dA = g->dBatch, *dI = dA + R * b.sA, *dP = dI + R * b.sI, *dPw = dP + R * b.sP, *dAl = dPw + R * b.sP,
           *dWv = dAl + R * b.sV, *dT = dWv + R * b.sV, *dT2 = dT + R * b.sT, *dS = dT2 + R * b.sT, *dDiag = dS + R * b.sS,
           *dJit = dDiag + R;
    KernParams *dKp = (KernParams *)g->dBatchAux;
    int *dInfo = (int *)(g->dBatchAux + kp_bytes);

    // per-member parameters: the context's kernel, dimension and Gower set-up with the member's variance / lengthscale(s)
    std::vector<KernParams> kp(R, g->kp);
    std::vector<double> diag(R), diag0(R), jit(R, 0.0);
    for (int r = 0; r < R; ++r) {
        kp[r].variance = variance[r];
        for (int d = 0; d < D; ++d) kp[r].ls[d] = g->ard ? lengthscale[(long)r * nls + d] : lengthscale[(long)r * nls];
        diag[r] = noise[r] + 1e-8;  // exact_gaussian_inference.py:56
        diag0[r] = (kp[r].gower ? std::pow(kp[r].variance, D) : kp[r].variance) + diag[r];
    }
    // the diagonal-tile kernel writes the lower block triangle of each inverted tile only: the blocks above it must be zero (as
    // set_data leaves the context's dInvL); the buffer is reused across calls of other shapes, so this is per call
    HIPCHK(hipMemsetAsync(dI, 0, sizeof(double) * b.sI * R, g->s));
    HIPCHK(hipMemcpyAsync(dKp, kp.data(), sizeof(KernParams) * R, hipMemcpyHostToDevice, g->s));
    HIPCHK(hipMemcpyAsync(dDiag, diag.data(), sizeof(double) * R, hipMemcpyHostToDevice, g->s));

    // jitter ladder per member (fit_impl, GPy/GPy/util/linalg.py:62-75): a member whose factorisation fails is factored again
    // with the next jitter, alone with the other failed members (runs of consecutive members share launches); the others keep
    // their factor
    std::vector<int> tries(R, 0), active(R, 1), st(R, 0), info(4 * R);
    for (int round = 0;; ++round) {
        if (round > 0) HIPCHK(hipMemcpyAsync(dJit, jit.data(), sizeof(double) * R, hipMemcpyHostToDevice, g->s));
        for (int m0 = 0; m0 < R;) {
            if (!active[m0]) {
                ++m0;
                continue;
            }
            int m1 = m0;
            while (m1 < R && active[m1]) ++m1;
            factor_members(g, b, dA, dI, dInfo, kp[m0], dKp, dDiag, dJit, m0, m1 - m0, round > 0);
            m0 = m1;
        }
        HIPCHK(hipMemcpyAsync(info.data(), dInfo, sizeof(int) * 4 * R, hipMemcpyDeviceToHost, g->s));
        GP_SYNC(g->s);
        bool again = false;
        for (int r = 0; r < R; ++r) {
            if (!active[r]) continue;
            const int inf = info[4 * r];
            if (inf == 0) {
                active[r] = 0;
                continue;
            }
            if (!(diag0[r] > 0.0)) {
                st[r] = GP_ERR_NOT_PD_DIAG;
                active[r] = 0;
                continue;
            }
            jit[r] = tries[r] == 0 ? diag0[r] * 1e-6 : jit[r] * 10.0;
            ++tries[r];
            if (tries[r] > maxtries || !std::isfinite(jit[r])) {
                st[r] = inf > 0 ? inf : 1;   // what gp_fit_grad returns for this member
                active[r] = 0;
                continue;
            }
            again = true;
        }
        if (!again) break;
    }

    // everything after the factorisation: all members in the same launches (a failed member's numbers are computed and dropped)
    const long Npad = b.Npad, lda = b.lda, PB = b.PB;
    const int nt = b.nt, W = b.W;
    // inverted diagonal panels (ensure_panel_inv: the solve of the identity against L_JJ, then one transpose)
    identity_blocks(g->s, dPw, PB, R * b.nJ);
    for (int J = 0; J < b.nJ; ++J) {
        const int J0 = J * W, Wp = std::min(W, nt - J0);
        double *Wb = dPw + (long)J * PB * PB;
        const double *Lb = dA + (long)J * (PB * lda + PB);
        const double *Ib = dI + (long)J0 * GP_TILE * GP_TILE;
        for (int bb = 0; bb < Wp; ++bb) {
            bgemm(g, 0, Wb, PB, Wb + (long)bb * GP_TILE, PB, Ib + (long)bb * GP_TILE * GP_TILE, GP_TILE, 0, GP_TILE,
                  TileSet{0, bb + 1, bb, bb + 1, 0}, inplace_opt(), R, b.sP, b.sP, b.sI);
            if (bb + 1 < Wp)
                bgemm(g, 1, Wb, PB, Wb + (long)bb * GP_TILE, PB, Lb + (long)bb * GP_TILE, lda, 1, GP_TILE,
                      TileSet{0, bb + 1, bb + 1, Wp, 0}, GemmOpt(), R, b.sP, b.sP, b.sA);
        }
    }
    launch_transpose_blocks(g->s, dP, dPw, PB, R * b.nJ);
    // log det, alpha = L^-T z, alpha . y (fit_impl's alpha_lml)
    launch_logdet_batch(g->s, dA, lda, b.sA, b.N, dS, b.sS, R);
    launch_trsv_backward_batch(g->s, dA, lda, b.sA, dP, b.sP, W, Npad, b.P, dAl, dWv, b.sV, R);
    launch_dot_ay_batch(g->s, dAl, b.sV, Npad, g->dY, b.N, b.P, dS + 8, b.sS, R);
    // L^-T into dT2 by the solve of the identity (solve_rows, trapezoid), then Ky^-1 = L^-T (L^-T)^T into dT (wi_lauum)
    identity_blocks(g->s, dT, Npad, R);
    for (int J0 = 0, J = 0; J0 < nt; ++J) {
        const int J1 = std::min(J0 + W, nt), rows = J1;
        GemmOpt o;
        o.k_end_tri = 1;
        o.b_sub = J0;
        bgemm(g, 0, dT2, Npad, dT + (long)J0 * GP_TILE, Npad, dP + (long)J * PB * PB, PB, 1, (J1 - J0) * GP_TILE,
              TileSet{0, rows, J0, J1, 0}, o, R, b.sT, b.sT, b.sP);
        if (J1 >= nt) break;
        bgemm(g, 1, dT, Npad, dT2 + (long)J0 * GP_TILE, Npad, dA + (long)J0 * GP_TILE, lda, 1, (J1 - J0) * GP_TILE,
              TileSet{0, rows, J1, nt, 0}, GemmOpt(), R, b.sT, b.sT, b.sA);
        J0 = J1;
    }
    HIPCHK(hipMemsetAsync(dT, 0, sizeof(double) * b.sT * R, g->s));
    if (g->lauum_panels) {
        for (int k0 = 0; k0 < nt; k0 += g->panel_tiles) {
            const int k1 = std::min(k0 + g->panel_tiles, nt);
            GemmOpt o;
            o.k_tri = 1;
            o.k_sub = k0;
            bgemm(g, 1, dT, Npad, dT2 + (long)k0 * GP_TILE, Npad, dT2 + (long)k0 * GP_TILE, Npad, 1, (k1 - k0) * GP_TILE,
                  TileSet{0, k1, 0, k1, 1}, o, R, b.sT, b.sT, b.sT);
        }
        launch_symmetrize_scale_batch(g->s, dT, b.sT, Npad, Npad, -1.0, R);
    } else {
        GemmOpt o;
        o.k_tri = 1;
        bgemm(g, 0, dT, Npad, dT2, Npad, dT2, Npad, 1, (int)Npad, TileSet{0, nt, 0, nt, 1}, o, R, b.sT, b.sT, b.sT);
        launch_symmetrize_scale_batch(g->s, dT, b.sT, Npad, Npad, 1.0, R);   // (x 1.0: the mirror of launch_symmetrize)
    }
    // the fused dL_dK reduction (lml_grad_impl), per-tile partials in dT2 (free after the product)
    int pass = 0;
    for (int d0 = 0; d0 < D; d0 += GP_GRAD_CH, ++pass) {
        launch_lml_grad_batch(g->s, g->dX, b.N, Npad, kp[0], dKp, g->ard, d0, dAl, b.sV, b.P, dT, b.sT, Npad, dT2, b.sT,
                              dS + 64 + pass * GP_GRAD_NACC, b.sS, R);
        if (!g->ard) break;
    }
    std::vector<double> sc((size_t)b.sS * R);
    HIPCHK(hipMemcpyAsync(sc.data(), dS, sizeof(double) * b.sS * R, hipMemcpyDeviceToHost, g->s));
    GP_SYNC(g->s);

    const double nan = std::nan("");
    const double log_2_pi = std::log(2.0 * M_PI);
    for (int r = 0; r < R; ++r) {
        status[r] = st[r];
        if (st[r]) {
            lml[r] = logdet[r] = jitter_used[r] = dvariance[r] = dnoise[r] = nan;
            for (int d = 0; d < nls; ++d) dlengthscale[(long)r * nls + d] = nan;
            continue;
        }
        const double *s = sc.data() + (size_t)b.sS * r;
        double fit = 0.0;
        for (int p = 0; p < b.P; ++p) fit += s[8 + p];
        logdet[r] = s[0];
        lml[r] = 0.5 * (-(double)b.N * b.P * log_2_pi - b.P * s[0] - fit);  // exact_gaussian_inference.py:62
        jitter_used[r] = jit[r];
        const double *h = s + 64;
        dvariance[r] = h[0] / kp[r].variance;  // stationary.py:224
        dnoise[r] = h[1];                      // gaussian.py:78-79
        if (g->ard) {
            for (int d = 0; d < D; ++d)
                dlengthscale[(long)r * nls + d] = -h[(d / GP_GRAD_CH) * GP_GRAD_NACC + 2 + (d % GP_GRAD_CH)] / kp[r].ls[d];
        } else {
            dlengthscale[(long)r * nls] = -h[2] / kp[r].ls[0];
        }
    }
    return 0;
}
