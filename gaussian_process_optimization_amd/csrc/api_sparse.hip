// The sparse GP: variational DTC inference over Mz inducing inputs Z, its gradients and its predictions, composed from the
// launchers the exact model is made of (K-build, tile Cholesky, inverted diagonal tiles, the NT GEMM on the fp64 MFMA,
// predict_grad) plus the kernels of sparse.hip.  See include/gphip.h, "sparse GP", for the contract of each entry point.
//
// Reference: VarDTC.inference, _compute_dL_dpsi, _compute_dL_dR, _compute_log_marginal_likelihood
// (GPy/GPy/inference/latent_function_inference/var_dtc.py:66-277; homoscedastic noise, certain inputs, no mean function),
// SparseGP.parameters_changed / _update_gradients (GPy/GPy/core/sparse_gp.py:76-119), the woodbury_inv prediction
// (posterior.py:225-248), GP.predictive_gradients over _predictive_variable = Z (GPy/GPy/core/gp.py:407-454).
//
// Data flow of a fit (n = Mzpad; every product is C = A B^T over each operand's contiguous dimension):
//   Kmm = K(Z) + 1e-8 I -> Lm (jitchol's ladder) -> Lm^-T by the solve of the identity (panel_inv_steps), Lm^-1 its transpose
//   Kfu [Npad, n] = launch_cross_k(X, Z);  V = Lm^-1 Kuf [n, Npad] (A = Lm^-1, B = Kfu);  VVt = V V^T (K = Npad: the O(N Mz^2) step)
//   B = I + beta VVt -> LB -> LB^-T, LB^-1
//   vectors [P][n]: beta V Y -> c1 = LB^-1 (.) (_LBi_Lmi_psi1Vf) -> LB^-T c1 -> w = Lm^-T (.) (Cpsi1Vf, the woodbury vector)
//   Dm = LB^-T (P I + c1 c1^T) LB^-1 (DBi_plus_BiPBi);  woodbury_inv = Lm^-T (I - LB^-T LB^-1) Lm^-1
//   gradients: dL_dKmm = Lm^-T (-0.5 Dm - 0.5 P B + P I) Lm^-1;  E = 0.5 Lm^-T (P I - Dm) Lm^-1 (dL_dpsi2_beta);  Wt = Kfu E;
//              launch_sparse_grad over (Z, Z; dL_dKmm) and over (Z, X; 2 beta Wt + beta Y w^T)
// S = L^-T M L^-1 (backsub_both_sides, linalg.py:381-390) is T = L^-T M (A = L^-T, B = M: M is symmetric), S = T L^-1 (A = T,
// B = L^-T).  In the padding (rows / columns >= Mz) Kmm and B are the identity and Kfu is zero, so the padded blocks of every
// factor and inverse are the identity and those of Dm, dL_dKmm, E and woodbury_inv decouple from the rows < Mz.
// Always true fp64: option "emulate_fp64" does not apply.
#include "api_internal.h"

// layout of sp.dOut (doubles)
enum { SPO_SCAL = 0, SPO_LOGDET = 8, SPO_TRACE = 10, SPO_HYP_NM = 16, SPO_HYP_MM = 16 + 4 * GP_SPARSE_NH, SPO_MIN = 16 + 8 * GP_SPARSE_NH,
       SPO_DZ = 160 };
static_assert(GP_MAX_D / GP_GRAD_CH * GP_SPARSE_NH <= 4 * GP_SPARSE_NH && SPO_MIN + 1 <= SPO_DZ, "sp.dOut: the slots do not overlap");

static int sparse_preamble(gp_ctx *g, bool need_z) {
    GP_DEAD_CHECK(g);
    GP_NO_MEAN(g, "the sparse entry points");
    if (!g->have_data || !g->have_params) return fail(GP_ERR_STATE, "set data and params before the sparse entry points");
    if (g->kp.gower) return fail(GP_ERR_STATE, "the sparse GP does not take the Gower option");
    if (g->warp.n > 0) return fail(GP_ERR_STATE, "the sparse GP does not take an output warp (gp_set_output_warp)");
    if (need_z && g->sp.Mz < 1) return fail(GP_ERR_STATE, "gp_sparse_set_inducing first");
    HIPCHK(hipSetDevice(g->device));
    return 0;
}

extern "C" int gp_sparse_set_inducing(gp_t *g, const double *Z, int64_t Mz) {
    if (!g || !Z) return fail(GP_ERR_ARG, "null argument");
    GP_DEAD_CHECK(g);
    GP_NO_MEAN(g, "gp_sparse_set_inducing");
    if (Mz < 1 || Mz > GP_SPARSE_MAX_INDUCING) return fail(GP_ERR_ARG, "Mz out of range (1..%d)", GP_SPARSE_MAX_INDUCING);
    if (!g->have_data) return fail(GP_ERR_STATE, "gp_set_data first");
    HIPCHK(hipSetDevice(g->device));
    GP_SYNC(g->s);
    SparseState &sp = g->sp;
    int rc;
    if ((rc = sp.dZ.reserve((long)GP_SPARSE_MAX_INDUCING * GP_MAX_D))) return rc;
    HIPCHK(hipMemcpy(sp.dZ, Z, sizeof(double) * Mz * g->D, hipMemcpyHostToDevice));
    sp.Mz = Mz;
    sp.Mzpad = round_up(Mz, GP_TILE);
    sparse_fit_dropped(g);
    return 0;
}

static int sparse_reserve(gp_ctx *g) {
    SparseState &sp = g->sp;
    const long n = sp.Mzpad, Npad = g->Npad;
    int rc;
    for (DevBuf<double> *b : {&sp.dKmm, &sp.dBm})
        if ((rc = b->reserve((n + GP_TILE) * n))) return rc;
    if ((rc = sp.dInvT.reserve(2 * n * GP_TILE))) return rc;
    for (DevBuf<double> *b : {&sp.dLmiT, &sp.dLmi, &sp.dLbiT, &sp.dLbi, &sp.dVVt, &sp.dDm, &sp.dE, &sp.dWinv, &sp.dDKmm, &sp.dTmp, &sp.dTmp2})
        if ((rc = b->reserve(n * n))) return rc;
    for (DevBuf<double> *b : {&sp.dKfu, &sp.dV, &sp.dWt})
        if ((rc = b->reserve(Npad * n))) return rc;
    if ((rc = sp.dVec.reserve(4L * g->P * n))) return rc;
    if ((rc = sp.dPartial.reserve(std::max(sparse_grad_partial_elems(n, g->N), sparse_grad_partial_elems(n, sp.Mz))))) return rc;
    if ((rc = sp.dOut.reserve(SPO_DZ + 2 * sp.Mz * g->D + g->N))) return rc;
    return sp.dInfo.reserve(4);
}

// the full n x n product C = A B^T
static void nt_square(gp_ctx *g, double *C, const double *A, const double *B, long n) {
    const int t = (int)(n / GP_TILE);
    gemm(g, g->s, 0, C, n, A, n, B, n, 1, (int)n, TileSet{0, t, 0, t, 0});
}
// S = L^-T M L^-1 from LiT = L^-T (M symmetric; tmp: n x n scratch)
static void both_sides(gp_ctx *g, double *S, const double *LiT, const double *M, double *tmp, long n) {
    nt_square(g, tmp, LiT, M, n);
    nt_square(g, S, tmp, LiT, n);
}

// jitchol (linalg.py:56-81) of the n x n matrix `build` writes into A ((n + 128) x n, lower tiles; one zero RHS tile row rides
// below), with the inverted diagonal tiles in invT; diag0: the mean of its diagonal, taken when the first attempt fails.
// Then LiT = L^-T (block upper triangular, zeros below).
template <class Build, class Diag0>
static int sparse_chol(gp_ctx *g, double *A, double *invT, double *LiT, Build build, Diag0 diag0, int maxtries, double *jitter_out) {
    SparseState &sp = g->sp;
    const long n = sp.Mzpad;
    const int ntz = (int)(n / GP_TILE);
    Members m;   // one member: the ladder of the batched fits (members_ladder) with nb = 1
    m.A = A;
    m.lda = n;
    m.invL = invT;
    m.info = sp.dInfo;
    std::vector<int> active(1, 1), st(1, 0);
    std::vector<double> jit(1, 0.0);
    // the diagonal-tile kernel writes the lower block triangle of each inverted tile only: the blocks above it must be zero
    HIPCHK(hipMemsetAsync(invT, 0, sizeof(double) * n * GP_TILE, g->s));
    int rc = members_ladder(g, m, ntz, maxtries, active, jit, nullptr, st,
                            [&](const Members &, int, bool jittered) {
                                build();
                                if (jittered) launch_add_diag(g->s, A, n, sp.Mz, jit[0]);
                                HIPCHK(hipMemsetAsync(A + n * n, 0, sizeof(double) * GP_TILE * n, g->s));
                                return 0;
                            },
                            [&](const std::vector<int> &, std::vector<double> &d0) { return diag0(&d0[0]); });
    if (rc || (rc = ladder_failure(st[0]))) return rc;
    *jitter_out = jit[0];
    launch_set_identity_blocks(g->s, LiT, n, 1);
    panel_inv_steps(g, g->s, LiT, n, A, n, invT, ntz, GemmOpt(), 0, 0);
    return 0;
}

static int sparse_fit_impl(gp_ctx *g, int maxtries) {
    SparseState &sp = g->sp;
    int rc;
    if ((rc = sparse_reserve(g))) return rc;
    sparse_fit_dropped(g);
    if (g->lap.on) fit_dropped(g);   // a regression fit clears the Laplace state: gp_set_params' noise is back before beta reads it
    const long n = sp.Mzpad, Mz = sp.Mz, N = g->N, Npad = g->Npad;
    const int P = g->P, ntz = (int)(n / GP_TILE), nt = (int)(Npad / GP_TILE);
    const double beta = 1.0 / std::max(g->noise, 1e-8);   // var_dtc.py:80
    hipStream_t s = g->s;
    double *vec0 = sp.dVec, *vec1 = vec0 + (long)P * n, *vec2 = vec1 + (long)P * n, *vec3 = vec2 + (long)P * n;

    // (the phases of the last call, for gp_last_phases: measurement only)
    g->nphases = 0;
    int ph = phase_begin(g, "sparse_kmm", (double)Mz * Mz * Mz * 2.0 / 3.0, 0.0);
    // Kmm = K(Z) + const_jitter I (var_dtc.py:93-95), Lm, Lm^-T, Lm^-1
    rc = sparse_chol(g, sp.dKmm, sp.dInvT, sp.dLmiT,
                     [&] { launch_kbuild(s, sp.dKmm, n, sp.dZ, Mz, n, g->kp, 1e-8, 0); },
                     [&](double *d0) { *d0 = g->kp.variance + 1e-8; return 0; }, maxtries, &sp.jitter_kmm);
    if (rc) {
        g->nphases = 0;   // (no half-recorded phase for gp_last_phases)
        return rc;
    }
    launch_transpose_blocks(s, sp.dLmi, sp.dLmiT, n, 1);
    phase_end(g, ph);
    ph = phase_begin(g, "sparse_kfu_v_vvt", 4.0 * (double)N * Mz * Mz, 8.0 * (double)N * Mz);
    // psi1 = K(X, Z) (var_dtc.py:125); V = Lm^-1 psi1^T (:130 without sqrt(beta)); A = beta V V^T (:131); B = I + A (:134)
    launch_cross_k(s, sp.dKfu, n, g->dX, N, Npad, sp.dZ, Mz, n, g->kp);
    gemm(g, s, 0, sp.dV, Npad, sp.dLmi, n, sp.dKfu, n, 1, (int)n, TileSet{0, ntz, 0, nt, 0});
    gemm(g, s, 0, sp.dVVt, n, sp.dV, Npad, sp.dV, Npad, 1, (int)Npad, TileSet{0, ntz, 0, ntz, 0});
    phase_end(g, ph);
    ph = phase_begin(g, "sparse_b", (double)Mz * Mz * Mz * 2.0 / 3.0, 0.0);
    rc = sparse_chol(g, sp.dBm, sp.dInvT + n * GP_TILE, sp.dLbiT,
                     [&] { launch_sparse_lincomb(s, sp.dBm, sp.dVVt, beta, nullptr, 0.0, 1.0, n); },
                     [&](double *d0) {   // mean diagonal of B = 1 + beta trace(VVt) / Mz
                         double tr[2];
                         launch_trace(s, sp.dVVt, n, Mz, sp.dOut + SPO_TRACE);
                         HIPCHK(hipMemcpyAsync(tr, sp.dOut + SPO_TRACE, sizeof tr, hipMemcpyDeviceToHost, s));
                         GP_SYNC(s);
                         *d0 = 1.0 + beta * tr[0] / (double)Mz;
                         return 0;
                     },
                     maxtries, &sp.jitter_b);
    if (rc) {
        g->nphases = 0;   // (no half-recorded phase for gp_last_phases)
        return rc;
    }
    launch_transpose_blocks(s, sp.dLbi, sp.dLbiT, n, 1);
    phase_end(g, ph);
    ph = phase_begin(g, "sparse_posterior", 12.0 * (double)Mz * Mz * Mz, 0.0);
    // _LBi_Lmi_psi1Vf, Cpsi1Vf (var_dtc.py:138-142), one row of n per output
    launch_sparse_thin(s, sp.dV, Npad, n, N, g->dY, 1, P, P, beta, vec0, n);
    launch_sparse_thin(s, sp.dLbi, n, n, n, vec0, n, 1, P, 1.0, vec1, n);
    launch_sparse_thin(s, sp.dLbiT, n, n, n, vec1, n, 1, P, 1.0, vec2, n);
    launch_sparse_thin(s, sp.dLmiT, n, n, n, vec2, n, 1, P, 1.0, vec3, n);
    // DBi_plus_BiPBi = LB^-T (P I + delit) LB^-1 (var_dtc.py:148-150)
    launch_sparse_outer(s, sp.dTmp, vec1, n, P, (double)P, n);
    both_sides(g, sp.dDm, sp.dLbiT, sp.dTmp, sp.dTmp2, n);
    launch_sparse_scalars(s, g->dY, N * P, sp.dVVt, sp.dDm, Mz, n, vec1, P, sp.dOut + SPO_SCAL);
    launch_logdet(s, sp.dBm, n, Mz, sp.dOut + SPO_LOGDET);
    // Bi = I - B^-1; woodbury_inv = Lm^-T Bi Lm^-1 (var_dtc.py:209-212)
    nt_square(g, sp.dTmp, sp.dLbiT, sp.dLbiT, n);
    launch_sparse_lincomb(s, sp.dTmp, sp.dTmp, -1.0, nullptr, 0.0, 1.0, n);
    both_sides(g, sp.dWinv, sp.dLmiT, sp.dTmp, sp.dTmp2, n);
    phase_end(g, ph);

    double sc[SPO_LOGDET + 1];
    HIPCHK(hipMemcpyAsync(sc, sp.dOut, sizeof sc, hipMemcpyDeviceToHost, s));
    GP_SYNC(s);
    const double trYYT = sc[0], trA = beta * sc[1], data_fit = sc[2], sumAD = beta * sc[3], logdetB = sc[SPO_LOGDET];
    const double psi0_sum = (double)N * g->kp.variance, NP = (double)N * P;
    // _compute_log_marginal_likelihood (var_dtc.py:266-277)
    const double lik_1 = -0.5 * NP * (std::log(2.0 * M_PI) - std::log(beta)) - 0.5 * beta * trYYT;
    const double lik_2 = -0.5 * P * (beta * psi0_sum - trA);
    const double lik_3 = -(double)P * 0.5 * logdetB;
    const double lik_4 = 0.5 * data_fit;
    sp.lml = lik_1 + lik_2 + lik_3 + lik_4;
    // _compute_dL_dR (var_dtc.py:261-263): the derivative with respect to the noise variance, also where the 1e-8 clamp is active
    double dR = -0.5 * NP * beta + 0.5 * trYYT * beta * beta;
    dR += 0.5 * P * (psi0_sum * beta * beta - trA * beta);
    dR += beta * (0.5 * sumAD - data_fit);
    sp.dnoise = dR;
    sp.beta = beta;
    sp.fitted = true;
    return 0;
}

extern "C" int gp_sparse_fit(gp_t *g, int maxtries, double *lml, double *jitter_kmm, double *jitter_b) {
    if (!g) return fail(GP_ERR_ARG, "null gp");
    int rc;
    if ((rc = sparse_preamble(g, true))) return rc;
    if ((rc = sparse_fit_impl(g, maxtries))) return rc;
    if (lml) *lml = g->sp.lml;
    if (jitter_kmm) *jitter_kmm = g->sp.jitter_kmm;
    if (jitter_b) *jitter_b = g->sp.jitter_b;
    return 0;
}

extern "C" int gp_sparse_fit_grad(gp_t *g, int maxtries, double *lml, double *dvariance, double *dlengthscale, double *dnoise, double *dZ) {
    if (!g || !dvariance || !dlengthscale || !dnoise || !dZ) return fail(GP_ERR_ARG, "null argument");
    int rc;
    if ((rc = sparse_preamble(g, true))) return rc;
    if (g->P > GP_SPARSE_GRAD_MAX_P) return fail(GP_ERR_ARG, "gp_sparse_fit_grad supports P <= %d", GP_SPARSE_GRAD_MAX_P);
    if (sparse_grad_lds_bytes(g->D, g->P) > (size_t)g->lds_per_wg)
        return fail(GP_ERR_ARG, "gp_sparse_fit_grad: D = %d, P = %d need %zu bytes of LDS per workgroup in the gradient pass, the device has %ld",
                    g->D, g->P, sparse_grad_lds_bytes(g->D, g->P), g->lds_per_wg);
    if ((rc = sparse_fit_impl(g, maxtries))) return rc;
    SparseState &sp = g->sp;
    const long n = sp.Mzpad, Mz = sp.Mz, N = g->N, Npad = g->Npad;
    const int P = g->P, D = g->D, ntz = (int)(n / GP_TILE), nt = (int)(Npad / GP_TILE);
    const double beta = sp.beta;
    hipStream_t s = g->s;
    const double *wv = sp.dVec + 3L * P * n;
    int ph = phase_begin(g, "sparse_grad_weights", 8.0 * (double)Mz * Mz * Mz + 2.0 * (double)N * Mz * Mz, 0.0);
    // dL_dKmm = Lm^-T (-0.5 DBi_plus_BiPBi - 0.5 P B + P I) Lm^-1 (var_dtc.py:152-156), B = I + beta VVt
    launch_sparse_lincomb(s, sp.dTmp, sp.dDm, -0.5, sp.dVVt, -0.5 * P * beta, 0.5 * P, n);
    both_sides(g, sp.dDKmm, sp.dLmiT, sp.dTmp, sp.dTmp2, n);
    // dL_dpsi2_beta = 0.5 Lm^-T (P I - DBi_plus_BiPBi) Lm^-1 (var_dtc.py:221); Wt = psi1 dL_dpsi2_beta (:232 without 2 beta)
    launch_sparse_lincomb(s, sp.dTmp, sp.dDm, -0.5, nullptr, 0.0, 0.5 * P, n);
    both_sides(g, sp.dE, sp.dLmiT, sp.dTmp, sp.dTmp2, n);
    gemm(g, s, 0, sp.dWt, n, sp.dKfu, n, sp.dE, n, 1, (int)n, TileSet{0, nt, 0, ntz, 0});
    phase_end(g, ph);
    double *dZmm = sp.dOut + SPO_DZ, *dZnm = dZmm + Mz * D;
    // the Kmm part (gradients_X's tmp + tmp.T: twice the symmetric weight), then the Knm part: dL_dKnm = beta Y w^T + 2 beta Wt
    ph = phase_begin(g, "sparse_grad_mm", 0.0, 8.0 * (double)Mz * Mz);
    launch_sparse_grad(s, sp.dZ, Mz, n, sp.dZ, Mz, g->kp, nullptr, 0, nullptr, 0, 0.0, sp.dDKmm, n, 1.0, sp.dPartial, 2.0, dZmm,
                       sp.dOut + SPO_HYP_MM);
    phase_end(g, ph);
    ph = phase_begin(g, "sparse_grad_nm", 0.0, 8.0 * (double)N * Mz);
    launch_sparse_grad(s, sp.dZ, Mz, n, g->dX, N, g->kp, g->dY, P, wv, n, beta, sp.dWt, n, 2.0 * beta, sp.dPartial, 1.0, dZnm,
                       sp.dOut + SPO_HYP_NM);
    phase_end(g, ph);
    std::vector<double> hyp((size_t)8 * GP_SPARSE_NH), dz((size_t)2 * Mz * D);
    HIPCHK(hipMemcpyAsync(hyp.data(), sp.dOut + SPO_HYP_NM, sizeof(double) * hyp.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(dz.data(), dZmm, sizeof(double) * dz.size(), hipMemcpyDeviceToHost, s));
    GP_SYNC(s);
    sp.grad_ready = true;
    const double *hnm = hyp.data(), *hmm = hyp.data() + 4 * GP_SPARSE_NH;
    // sparse_gp.py:110-115: the diagonal part (dL_dKdiag = -0.5 P beta per row: variance only), the Knm part, the Kmm part
    *dvariance = -0.5 * P * beta * (double)N + hnm[0] / g->kp.variance + hmm[0] / g->kp.variance;   // stationary.py:224
    double iso = 0.0;
    for (int d = 0; d < D; ++d) {   // -sum W g d_q^2 / l_q (stationary.py:230-238)
        const int at = (d / GP_GRAD_CH) * GP_SPARSE_NH + 1 + d % GP_GRAD_CH;
        const double v = -hnm[at] / g->kp.ls[d] + -hmm[at] / g->kp.ls[d];
        if (g->ard) dlengthscale[d] = v;
        iso += v;
    }
    if (!g->ard) dlengthscale[0] = iso;
    *dnoise = sp.dnoise;
    // sparse_gp.py:117-118
    for (long e = 0; e < Mz * D; ++e) dZ[e] = dz[e] + dz[Mz * D + e];
    if (lml) *lml = sp.lml;
    return 0;
}

int sparse_fitted(gp_ctx *g) {
    int rc;
    if ((rc = sparse_preamble(g, true))) return rc;
    GP_NO_LAPLACE(g, "the sparse model's entries");   // (they read the context's noise, which is 1 in that state; gp_sparse_fit clears it)
    if (!g->sp.fitted) return fail(GP_ERR_STATE, "gp_sparse_fit first");
    return 0;
}

extern "C" int gp_sparse_posterior(gp_t *g, double *woodbury_vector, double *woodbury_inv) {
    if (!g || (!woodbury_vector && !woodbury_inv)) return fail(GP_ERR_ARG, "null argument");
    int rc;
    if ((rc = sparse_fitted(g))) return rc;
    SparseState &sp = g->sp;
    const long n = sp.Mzpad, Mz = sp.Mz;
    const int P = g->P;
    if (woodbury_vector) {
        std::vector<double> rows((size_t)P * n);
        HIPCHK(hipMemcpyAsync(rows.data(), sp.dVec + 3L * P * n, sizeof(double) * rows.size(), hipMemcpyDeviceToHost, g->s));
        GP_SYNC(g->s);
        for (long m = 0; m < Mz; ++m)
            for (int p = 0; p < P; ++p) woodbury_vector[m * P + p] = rows[(size_t)p * n + m];
    }
    if (woodbury_inv) {
        GP_SYNC(g->s);
        HIPCHK(hipMemcpy2D(woodbury_inv, sizeof(double) * Mz, sp.dWinv, sizeof(double) * n, sizeof(double) * Mz, Mz,
                           hipMemcpyDeviceToHost));
    }
    return 0;
}

// Posterior._raw_predict (posterior.py:225-248) and GP.predictive_gradients (gp.py:407-454) over the M rows at dX (device, [M, D]):
// mean [M, P], var [M] and, with grads, dmdx [M, D, P] and dvdx [M, D], all on the device.  THE arithmetic of every posterior the
// sparse entries serve outside the fused rows path -- gp_sparse_predict, the resident table's cache, the rows entries' fallback --:
// chunks of "mc_max" rows, one pinned GEMM instance, one reduce, so that a row has the same bits wherever it is predicted.
static int sparse_posterior_rows(gp_ctx *g, const double *dX, long M, int include_noise, bool grads, double *dmean, double *dvar,
                                 double *ddm, double *ddv) {
    SparseState &sp = g->sp;
    const long n = sp.Mzpad, Mz = sp.Mz;
    const int P = g->P, D = g->D, ntz = (int)(n / GP_TILE);
    const long mc_max = std::min(round_up(g->mc_max, GP_TILE), round_up(M, GP_TILE));
    hipStream_t s = g->s;
    int rc;
    if ((rc = sp.dKx.reserve(mc_max * n))) return rc;
    if ((rc = sp.dBt.reserve(mc_max * n))) return rc;
    const double *wv = sp.dVec + 3L * P * n;
    // the product with woodbury_inv always runs as 64 x 64 work units: ONE GEMM instance whatever the table's size, so that a
    // row's posterior does not depend on the rows it is predicted with (include/gphip.h)
    GemmOpt pinned;
    pinned.small = 1;
    for (long m0 = 0; m0 < M; m0 += mc_max) {
        const long mc = std::min(mc_max, (long)M - m0), mcpad = round_up(mc, GP_TILE);
        launch_cross_k(s, sp.dKx, n, dX + m0 * D, mc, mcpad, sp.dZ, Mz, n, g->kp);
        // Bt = Kx woodbury_inv (woodbury_inv symmetric: its rows serve as the B operand)
        launch_gemm_nt(s, 0, sp.dBt, n, sp.dKx, n, sp.dWinv, n, 1, (int)n, TileSet{0, (int)(mcpad / GP_TILE), 0, ntz, 0}, pinned);
        launch_sparse_predict_reduce(s, sp.dKx, sp.dBt, n, mc, Mz, wv, n, P, g->kp.variance, include_noise ? g->noise : 0.0,
                                     dmean + m0 * P, dvar + m0);
        // gp.py:432-453 with _predictive_variable = Z: gradients_X(w_p^T, Xs, Z) and gradients_X(-2 Kx woodbury_inv, Xs, Z)
        if (grads) launch_predict_grad(s, dX + m0 * D, mc, sp.dZ, Mz, g->kp, wv, n, P, sp.dBt, n, ddm + m0 * D * P, ddv + m0 * D);
    }
    return 0;
}

extern "C" int gp_sparse_predict(gp_t *g, const double *Xs, int64_t M, int include_noise, double *mean, double *var, double *dmdx,
                                 double *dvdx) {
    if (!g || !Xs || !mean || !var) return fail(GP_ERR_ARG, "null argument");
    if (M < 1) return fail(GP_ERR_ARG, "M < 1");
    int rc;
    if ((rc = sparse_fitted(g))) return rc;
    SparseState &sp = g->sp;
    const int P = g->P, D = g->D;
    const bool grads = dmdx || dvdx;
    hipStream_t s = g->s;
    if ((rc = sp.dXs.reserve(M * D))) return rc;
    if ((rc = sp.dPred.reserve(M * (P + 1 + (long)D * P + D)))) return rc;
    double *dmean = sp.dPred, *dvar = dmean + M * P, *ddm = dvar + M, *ddv = ddm + M * D * P;
    HIPCHK(hipMemcpyAsync(sp.dXs, Xs, sizeof(double) * M * D, hipMemcpyHostToDevice, s));
    g->nphases = 0;
    int ph = phase_begin(g, "sparse_predict", 2.0 * (double)M * sp.Mz * sp.Mz, 8.0 * (double)M * sp.Mz);
    if ((rc = sparse_posterior_rows(g, sp.dXs, M, include_noise, grads, dmean, dvar, ddm, ddv))) return rc;
    phase_end(g, ph);
    HIPCHK(hipMemcpyAsync(mean, dmean, sizeof(double) * M * P, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(var, dvar, sizeof(double) * M, hipMemcpyDeviceToHost, s));
    if (dmdx) HIPCHK(hipMemcpyAsync(dmdx, ddm, sizeof(double) * M * D * P, hipMemcpyDeviceToHost, s));
    if (dvdx) HIPCHK(hipMemcpyAsync(dvdx, ddv, sizeof(double) * M * D, hipMemcpyDeviceToHost, s));
    GP_SYNC(s);
    return 0;
}

extern "C" int gp_sparse_fmin(gp_t *g, double *fmin) {
    if (!g || !fmin) return fail(GP_ERR_ARG, "null argument");
    int rc;
    if ((rc = sparse_fitted(g))) return rc;
    SparseState &sp = g->sp;
    const long n = sp.Mzpad, Mz = sp.Mz, N = g->N;
    if (sp.fmin_valid) {   // cached per fit, as gp_fmin: the acquisitions ask for it with every call
        *fmin = sp.fmin;
        return 0;
    }
    double *mu = sp.dOut + SPO_DZ + 2 * Mz * g->D;
    // the posterior mean at the training inputs, psi1 w (first output column), and its minimum (gpmodel.py:125-129)
    launch_sparse_thin(g->s, sp.dKfu, n, N, Mz, sp.dVec + 3L * g->P * n, n, 1, 1, 1.0, mu, N);
    launch_sparse_min(g->s, mu, N, sp.dOut + SPO_MIN);
    HIPCHK(hipMemcpyAsync(&sp.fmin, sp.dOut + SPO_MIN, sizeof(double), hipMemcpyDeviceToHost, g->s));
    GP_SYNC(g->s);
    sp.fmin_valid = true;
    *fmin = sp.fmin;
    return 0;
}

// ---- acquisitions over the sparse model's resident candidate table ----------------------------------------------------------------
// gp_acq* of the exact model restated over the sparse posterior: the table lives in sp.dTab, its posterior (noise included, as
// GPModel.predict asks, gpmodel.py:102) is cached in sp.dTabPost until the sparse fit is dropped, and the scoring, penalising,
// masking and reducing launchers are the exact model's, on buffers of the sparse model's own.
extern "C" int gp_sparse_set_candidates(gp_t *g, const double *Xs, int64_t M) {
    if (!g || !Xs) return fail(GP_ERR_ARG, "null argument");
    GP_DEAD_CHECK(g);
    GP_NO_MEAN(g, "gp_sparse_set_candidates");
    if (M < 1) return fail(GP_ERR_ARG, "M < 1");
    if (!g->have_data) return fail(GP_ERR_STATE, "gp_set_data first");
    HIPCHK(hipSetDevice(g->device));
    GP_SYNC(g->s);
    SparseState &sp = g->sp;
    int rc;
    if ((rc = sp.dTab.reserve(M * g->D))) return rc;
    HIPCHK(hipMemcpy(sp.dTab, Xs, sizeof(double) * M * g->D, hipMemcpyHostToDevice));
    sp.tM = M;
    sp.tab_post = sp.tab_grad = false;
    if (g->cost_tab == 2) g->cost_tab = 0;
    return 0;
}

// what every scoring entry asks first: a sparse fit, a single output, a known acquisition, a sound batch, a table
static int sparse_scoring(gp_ctx *g, const AcqSpec &a, const LpSpec *lp) {
    int rc;
    if ((rc = sparse_fitted(g))) return rc;
    if ((rc = check_acq(g, a, lp))) return rc;
    if (lp && (rc = check_lp(*lp))) return rc;
    if (g->sp.tM < 1) return fail(GP_ERR_STATE, "gp_sparse_set_candidates first");
    return 0;
}

// mean / var (and, with grads, the gradients) of the resident table in sp.dTabPost: the bits gp_sparse_predict(include_noise = 1)
// returns for those rows
static int sparse_table_posterior(gp_ctx *g, bool grads) {
    SparseState &sp = g->sp;
    if (sp.tab_post && (!grads || sp.tab_grad)) return 0;
    const long M = sp.tM, D = g->D;
    int rc;
    if (sp.dTabPost.cap < M * (2 + 2 * D)) sp.tab_post = sp.tab_grad = false;   // (reserve does not keep the contents)
    if ((rc = sp.dTabPost.reserve(M * (2 + 2 * D)))) return rc;
    double *dmean = sp.dTabPost, *dvar = dmean + M, *ddm = dvar + M, *ddv = ddm + M * D;
    if ((rc = sparse_posterior_rows(g, sp.dTab, M, 1, grads, dmean, dvar, ddm, ddv))) return rc;
    sp.tab_post = true;
    sp.tab_grad = sp.tab_grad || grads;
    return 0;
}

// scores of `M` rows at dX from their posterior at post (layout of sp.dTabPost) into acq [M] (and dacq [M, D] with grad)
static int sparse_scores(gp_ctx *g, const AcqSpec &a, const LpSpec *lp, bool grad, const double *dX, long M, const double *post,
                         double *acq, double *dacq) {
    const double *dmean = post, *dvar = dmean + M, *ddm = dvar + M, *ddv = ddm + M * g->D;
    return score_rows(g, a, lp, grad, ScoreRows{dX, M, dmean, dvar, ddm, ddv, acq, dacq});
}

static int sparse_table_scores(gp_ctx *g, const AcqSpec &a, const LpSpec *lp, bool grad) {
    SparseState &sp = g->sp;
    int rc;
    if ((rc = sparse_table_posterior(g, grad))) return rc;
    if ((rc = sp.dTabAcq.reserve(sp.tM))) return rc;
    if (grad && (rc = sp.dTabDacq.reserve(sp.tM * g->D))) return rc;
    return sparse_scores(g, a, lp, grad, sp.dTab, sp.tM, sp.dTabPost, sp.dTabAcq, sp.dTabDacq);
}

extern "C" int gp_sparse_acq(gp_t *g, int type, double par, double fmin, double y_mean, double y_std, int lp, int transform,
                             const double *Xb, int nb, const double *r_x0, const double *s_x0, double *out, double *dout) {
    if (!g || !out) return fail(GP_ERR_ARG, "null argument");
    const AcqSpec a{type, par, fmin, y_mean, y_std};
    const LpSpec batch{transform, Xb, nb, r_x0, s_x0}, *pen = lp ? &batch : nullptr;
    int rc;
    if ((rc = sparse_scoring(g, a, pen))) return rc;
    if ((rc = sparse_table_scores(g, a, pen, dout != nullptr))) return rc;
    return scores_out(g, g->sp.dTabAcq, g->sp.dTabDacq, g->sp.tM, g->D, out, dout);
}

extern "C" int gp_sparse_acq_argbest(gp_t *g, int type, double par, double fmin, double y_mean, double y_std, int lp, int transform,
                                     const double *Xb, int nb, const double *r_x0, const double *s_x0, int sense,
                                     const int64_t *exclude, int nex, int64_t *idx, double *val) {
    if (!g || !idx || !val) return fail(GP_ERR_ARG, "null argument");
    const AcqSpec a{type, par, fmin, y_mean, y_std};
    const LpSpec batch{transform, Xb, nb, r_x0, s_x0}, *pen = lp ? &batch : nullptr;
    int rc;
    if ((rc = sparse_scoring(g, a, pen))) return rc;
    if ((rc = check_sense(sense))) return rc;
    if ((rc = check_exclude(exclude, nex, g->sp.tM))) return rc;
    if ((rc = sparse_table_scores(g, a, pen, false))) return rc;
    return select_best(g, g->sp.dTabAcq, g->sp.tM, sense, exclude, nex, idx, val);
}

extern "C" int gp_sparse_acq_topk(gp_t *g, int type, double par, double fmin, double y_mean, double y_std, int sense, int k,
                                  int64_t *idx, double *val) {
    if (!g || !idx || !val) return fail(GP_ERR_ARG, "null argument");
    const AcqSpec a{type, par, fmin, y_mean, y_std};
    int rc;
    if ((rc = sparse_scoring(g, a, nullptr))) return rc;
    if ((rc = check_sense(sense))) return rc;
    if ((rc = check_k(k))) return rc;
    if ((rc = sparse_table_scores(g, a, nullptr, false))) return rc;
    return select_topk(g, g->sp.dTabAcq, g->sp.tM, sense, k, idx, val);
}

// ---- a handful of locations per call (csrc/sparse_rows.hip) -------------------------------------------------------------------------
// fused path: up to min("small_m", ROWS_WIDE_M) locations of a single-output model; a pass takes as many of them as fit the kernel
// arguments (M D <= ROWS_MAX_XS: all eight up to D = 16, two at D = GP_MAX_D).  A location's bits do not depend on the split.
static bool sparse_rows_fused_ok(const gp_ctx *g, int64_t M) {
    return g->small_m > 0 && M >= 1 && M <= std::min<long>(g->small_m, ROWS_WIDE_M) && g->P == 1;
}

static int sparse_rows_scratch(gp_ctx *g) {
    SparseState &sp = g->sp;
    int rc;
    if ((rc = sp.dRowsPart.reserve((long)sparse_rows_grid(GP_SPARSE_MAX_INDUCING) * SPARSE_ROWS_GROW))) return rc;
    if ((rc = sp.pass.ready(g->s))) return rc;
    if (!sp.zs_valid) {   // Z / lengthscale, once per fit and only for models that come here
        if ((rc = sp.dZs.reserve(sp.Mz * g->D))) return rc;
        launch_sparse_scale_z(g->s, sp.dZ, sp.Mz, g->kp, sp.dZs);
        sp.zs_valid = true;
    }
    return 0;
}

// mode as launch_sparse_rows.  Results: mean / var / acq [M], dmdx / dvdx / dacq [M, D] (any may be null).
static int sparse_rows_fused(gp_ctx *g, const double *Xs, int M, int mode, int include_noise, const RowsAcq &aq, double *mean,
                             double *var, double *acq, double *dmdx, double *dvdx, double *dacq, bool per_cost = false) {
    SparseState &sp = g->sp;
    int rc;
    if ((rc = sparse_rows_scratch(g))) return rc;
    const int D = g->D;
    const double *wv = sp.dVec + 3L * g->P * sp.Mzpad;
    rc = rows_passes(
        g, sp.pass, Xs, M, std::min(M, ROWS_MAX_XS / D),
        [&](const RowsX &rx, const PassReport &r, unsigned *arrivals) {
            launch_sparse_rows(g->s, sp.dWinv, sp.Mzpad, sp.Mz, rx, g->kp, sp.dZs, wv, mode, g->kp.variance,
                               include_noise ? g->noise : 0.0, aq, sp.dRowsPart, r);
            if (per_cost) cost_divide_block(g, rx, mode == 1, r.out, ROWS_WIDE_M);   // behind the pass, before the drain
            arrivals[0] = sparse_rows_grid(sp.Mz);
            return 0;
        },
        [&](int m0, int mc, const double *o) { rows_unpack(o, ROWS_WIDE_M, m0, mc, D, mean, var, acq, dmdx, dvdx, dacq); });
    if (!rc) ++sp.rows_fused_calls;
    return rc;
}

// Everything the fused path does not take: the table arithmetic on scratch buffers (never the resident table or its cache).
static int sparse_rows_fallback(gp_ctx *g, const double *Xs, long M, int include_noise, bool grads, const AcqSpec *a, const LpSpec *lp,
                                double *mean, double *var, double *acq, double *dmdx, double *dvdx, double *dacq) {
    SparseState &sp = g->sp;
    const long D = g->D;
    hipStream_t s = g->s;
    int rc;
    ++sp.rows_fallback_calls;
    if ((rc = sp.dScrX.reserve(M * D))) return rc;
    if ((rc = sp.dScrPost.reserve(M * (2 + 2 * D)))) return rc;
    if ((rc = sp.dScrAcq.reserve(M * (1 + D)))) return rc;
    double *dmean = sp.dScrPost, *dvar = dmean + M, *ddm = dvar + M, *ddv = ddm + M * D, *dacq_d = sp.dScrAcq + M;
    HIPCHK(hipMemcpyAsync(sp.dScrX, Xs, sizeof(double) * M * D, hipMemcpyHostToDevice, s));
    if ((rc = sparse_posterior_rows(g, sp.dScrX, M, include_noise, grads, dmean, dvar, ddm, ddv))) return rc;
    if (a && (rc = sparse_scores(g, *a, lp, grads, sp.dScrX, M, sp.dScrPost, sp.dScrAcq, dacq_d))) return rc;
    if (mean) HIPCHK(hipMemcpyAsync(mean, dmean, sizeof(double) * M, hipMemcpyDeviceToHost, s));
    if (var) HIPCHK(hipMemcpyAsync(var, dvar, sizeof(double) * M, hipMemcpyDeviceToHost, s));
    if (dmdx) HIPCHK(hipMemcpyAsync(dmdx, ddm, sizeof(double) * M * D, hipMemcpyDeviceToHost, s));
    if (dvdx) HIPCHK(hipMemcpyAsync(dvdx, ddv, sizeof(double) * M * D, hipMemcpyDeviceToHost, s));
    return scores_out(g, sp.dScrAcq, dacq_d, M, g->D, acq, dacq);
}

extern "C" int gp_sparse_predict_rows(gp_t *g, const double *Xs, int64_t M, int include_noise, double *mean, double *var, double *dmdx,
                                      double *dvdx) {
    if (!g || !Xs) return fail(GP_ERR_ARG, "null argument");
    int rc;
    if ((rc = sparse_fitted(g))) return rc;
    if (g->P != 1) return fail(GP_ERR_ARG, "the rows entries need P == 1");
    if (M < 1) return fail(GP_ERR_ARG, "M < 1");
    if (dvdx && !dmdx) return fail(GP_ERR_ARG, "dvdx needs dmdx");
    if (dmdx && !dvdx && (mean || var)) return fail(GP_ERR_ARG, "the mean's gradient alone (dvdx NULL) comes without mean / var");
    const int mode = !dmdx ? 0 : dvdx ? 1 : 2;
    if (sparse_rows_fused_ok(g, M)) {
        RowsAcq aq{};
        return sparse_rows_fused(g, Xs, (int)M, mode, include_noise, aq, mean, var, nullptr, dmdx, dvdx, nullptr);
    }
    return sparse_rows_fallback(g, Xs, M, include_noise, dmdx != nullptr, nullptr, nullptr, mean, var, nullptr, dmdx, dvdx, nullptr);
}

extern "C" int gp_sparse_acq_rows(gp_t *g, const double *Xs, int64_t M, int type, double par, double fmin, double y_mean, double y_std,
                                  int lp, int transform, const double *Xb, int nb, const double *r_x0, const double *s_x0, double *out,
                                  double *dout) {
    if (!g || !Xs || !out) return fail(GP_ERR_ARG, "null argument");
    int rc;
    if ((rc = sparse_fitted(g))) return rc;
    if (M < 1) return fail(GP_ERR_ARG, "M < 1");
    const AcqSpec a{type, par, fmin, y_mean, y_std};
    const LpSpec batch{transform, Xb, nb, r_x0, s_x0}, *pen = lp ? &batch : nullptr;
    if ((rc = check_acq(g, a, pen))) return rc;
    if (pen && (rc = check_lp(*pen))) return rc;
    if (sparse_rows_fused_ok(g, M)) {
        LpBatch b;
        if (pen && (rc = rows_lp_batch(g, *pen, &b))) return rc;   // (keeps the shared batch cache in step with dLp)
        return sparse_rows_fused(g, Xs, (int)M, dout ? 1 : 0, 1, rows_acq(a, pen, b), nullptr, nullptr, out, nullptr, nullptr,
                                 dout, acq_per_cost(type));   // with_noise=True, gpmodel.py:102
    }
    return sparse_rows_fallback(g, Xs, M, 1, dout != nullptr, &a, pen, nullptr, nullptr, out, nullptr, nullptr, dout);
}

// how many sparse rows calls took the fused path / the table arithmetic since the context was created (route checks in tests)
extern "C" int gp_sparse_rows_stats(gp_t *g, int64_t *fused, int64_t *fallback) {
    if (!g) return fail(GP_ERR_ARG, "null gp");
    if (fused) *fused = g->sp.rows_fused_calls;
    if (fallback) *fallback = g->sp.rows_fallback_calls;
    return 0;
}
