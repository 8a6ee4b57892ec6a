// The sparse GP's JOINT posterior: full covariance, posterior samples and the covariance against a resident second point set.
// See include/gphip.h, "sparse GP", for the contract of each entry point.
//
// Reference: Posterior._raw_predict with full_cov (posterior.py:229-232) over _predictive_variable = Z,
//     cov = K(Xs, Xs) - K(Xs, Z) woodbury_inv K(Z, Xs),
// the likelihood's noise on the diagonal (gaussian.py:104-105), GP.posterior_samples_f (gp.py:581-609).
//
// The covariance is formed in the FACTORED form.  With woodbury_inv = Lm^-T (I - B^-1) Lm^-1 and B = LB LB^T,
//     U = K(Xs, Z) Lm^-T,   T = U LB^-T,   cov = K(Xs, Xs) - U U^T + T T^T:
// K(Xs, Xs) - U U^T is the Nystroem residual of the prior and T T^T the part the data give back, both positive semi-definite, so
// that most of the cancellation of the reference's single subtraction never happens.  Two products A A^T on the fp64 GEMM, lower
// tiles only, mirrored: the matrix is bitwise symmetric.  Everything runs on buffers of SparseState's own (sp.dCov*): the exact
// model's candidates, posterior and covariance scratch, the sparse table cache and the cost snapshot are not touched.
//
// gp_sparse_cov_between works from G = K(X2, Z) woodbury_inv of the resident second point set, cached per fit (csrc/sparse_cov.hip).
#include "api_internal.h"

// U into sp.dCovU, T into sp.dCovA and the mean (one row of Mpad per output) into sp.dCovMean, for the M rows at sp.dCovX
static int cov_factors(gp_ctx *g, long M) {
    SparseState &sp = g->sp;
    const long n = sp.Mzpad, Mz = sp.Mz, Mpad = round_up(M, GP_TILE);
    const int P = g->P, ntz = (int)(n / GP_TILE), mt = (int)(Mpad / GP_TILE);
    hipStream_t s = g->s;
    int rc;
    if ((rc = sp.dCovA.reserve(Mpad * n))) return rc;
    if ((rc = sp.dCovU.reserve(Mpad * n))) return rc;
    if ((rc = sp.dCovMean.reserve((long)P * Mpad))) return rc;
    launch_cross_k(s, sp.dCovA, n, sp.dCovX, M, Mpad, sp.dZ, Mz, n, g->kp);
    launch_sparse_thin(s, sp.dCovA, n, M, Mz, sp.dVec + 3L * P * n, n, 1, P, 1.0, sp.dCovMean, Mpad);   // mean = Kx w
    gemm(g, s, 0, sp.dCovU, n, sp.dCovA, n, sp.dLmi, n, 1, (int)n, TileSet{0, mt, 0, ntz, 0});   // U = Kx Lm^-T (B: the rows of Lm^-1)
    gemm(g, s, 0, sp.dCovA, n, sp.dCovU, n, sp.dLbi, n, 1, (int)n, TileSet{0, mt, 0, ntz, 0});   // T = U LB^-T
    return 0;
}

// sp.dCovC = K(Xs, Xs) - U U^T + T T^T (+ noise on the diagonal), Mpad x Mpad with the identity in the padding
static int cov_build(gp_ctx *g, long M, int include_noise) {
    SparseState &sp = g->sp;
    const long n = sp.Mzpad, Mpad = round_up(M, GP_TILE);
    const int mt = (int)(Mpad / GP_TILE);
    hipStream_t s = g->s;
    int rc;
    if ((rc = sp.dCovC.reserve(Mpad * Mpad))) return rc;
    if ((rc = sp.dCovW.reserve(Mpad * Mpad))) return rc;
    launch_kbuild(s, sp.dCovC, Mpad, sp.dCovX, M, Mpad, g->kp, 0.0, 1);
    gemm(g, s, 1, sp.dCovC, Mpad, sp.dCovU, n, sp.dCovU, n, 1, (int)n, TileSet{0, mt, 0, mt, 1});
    gemm(g, s, 0, sp.dCovW, Mpad, sp.dCovA, n, sp.dCovA, n, 1, (int)n, TileSet{0, mt, 0, mt, 1});
    launch_sparse_lincomb(s, sp.dCovC, sp.dCovC, 1.0, sp.dCovW, 1.0, 0.0, Mpad);
    launch_symmetrize(s, sp.dCovC, Mpad, Mpad);   // (the tiles above the diagonal were never formed)
    if (include_noise) launch_add_diag(s, sp.dCovC, Mpad, M, g->noise);   // gaussian.py:104-105
    return 0;
}

// what the two entries over a prediction set ask first; on success Xs is on its way to sp.dCovX
static int cov_preamble(gp_ctx *g, const double *Xs, int64_t M, const char *who) {
    if (M < 1) return fail(GP_ERR_ARG, "M < 1");
    int rc;
    if ((rc = sparse_fitted(g))) return rc;
    if (round_up(M, GP_TILE) > g->mc_max) return fail(GP_ERR_ARG, "%s needs M <= mc_max (%ld)", who, g->mc_max);
    if ((rc = g->sp.dCovX.reserve(M * g->D))) return rc;
    HIPCHK(hipMemcpyAsync(g->sp.dCovX, Xs, sizeof(double) * M * g->D, hipMemcpyHostToDevice, g->s));
    return 0;
}

// mean [M, P] from the rows of sp.dCovMean (drains the stream)
static int cov_mean_out(gp_ctx *g, long M, double *mean) {
    const long Mpad = round_up(M, GP_TILE);
    const int P = g->P;
    std::vector<double> rows((size_t)P * Mpad);
    HIPCHK(hipMemcpyAsync(rows.data(), g->sp.dCovMean, sizeof(double) * rows.size(), hipMemcpyDeviceToHost, g->s));
    GP_SYNC(g->s);
    for (long m = 0; m < M; ++m)
        for (int p = 0; p < P; ++p) mean[m * P + p] = rows[(size_t)p * Mpad + m];
    return 0;
}

extern "C" int gp_sparse_predict_full_cov(gp_t *g, const double *Xs, int64_t M, int include_noise, double *mean, double *cov) {
    if (!g || !Xs || !cov) return fail(GP_ERR_ARG, "null argument");
    int rc;
    if ((rc = cov_preamble(g, Xs, M, "the full covariance"))) return rc;
    SparseState &sp = g->sp;
    const long Mpad = round_up(M, GP_TILE);
    if ((rc = cov_factors(g, M))) return rc;
    if ((rc = cov_build(g, M, include_noise))) return rc;
    if (mean && (rc = cov_mean_out(g, M, mean))) return rc;
    GP_SYNC(g->s);
    HIPCHK(hipMemcpy2D(cov, sizeof(double) * M, sp.dCovC, sizeof(double) * Mpad, sizeof(double) * M, M, hipMemcpyDeviceToHost));
    return 0;
}

// gp_posterior_samples (api_predict.hip) over the sparse covariance: the M x M Cholesky on the device with the tile kernels of the
// fit (factor_buf) under jitchol's ladder (linalg.py:56-81, ladder_step), then dev = Z C^T by the product that ends at the diagonal
extern "C" int gp_sparse_posterior_samples(gp_t *g, const double *Xs, int64_t M, int include_noise, const double *Z, int S, int maxtries,
                                           double *mean, double *dev, double *jitter_used) {
    if (!g || !Xs || !Z || !dev) return fail(GP_ERR_ARG, "null argument");
    if (S < 1) return fail(GP_ERR_ARG, "S < 1");
    int rc;
    if ((rc = cov_preamble(g, Xs, M, "posterior samples"))) return rc;
    SparseState &sp = g->sp;
    const long Mpad = round_up(M, GP_TILE), Spad = round_up(S, GP_TILE);
    const int mt = (int)(Mpad / GP_TILE), st = (int)(Spad / GP_TILE);
    hipStream_t s = g->s;
    if ((rc = sp.dCovZ.reserve(2 * Spad * Mpad))) return rc;
    if ((rc = sp.dCovInv.reserve(Mpad * GP_TILE))) return rc;
    if ((rc = sp.dCovStat.reserve(2))) return rc;
    double *Zd = sp.dCovZ, *Dv = Zd + Spad * Mpad;
    HIPCHK(hipMemsetAsync(Zd, 0, sizeof(double) * Spad * Mpad, s));
    HIPCHK(hipMemcpy2DAsync(Zd, sizeof(double) * Mpad, Z, sizeof(double) * M, sizeof(double) * M, S, hipMemcpyHostToDevice, s));
    // (the diagonal-tile kernel writes the lower block triangle of an inverted tile only)
    HIPCHK(hipMemsetAsync(sp.dCovInv, 0, sizeof(double) * Mpad * GP_TILE, s));
    if ((rc = cov_factors(g, M))) return rc;
    // jitchol scales its ladder by the mean of the diagonal of the matrix it factors (linalg.py:62-66): the POSTERIOR covariance
    double diag_stat[2] = {0.0, 0.0};   // trace and smallest entry of its diagonal
    double jitter = 0.0;
    int tries = 0;
    for (int info = 0;;) {
        if ((rc = cov_build(g, M, include_noise))) return rc;
        if (tries == 0) {
            launch_trace(s, sp.dCovC, Mpad, M, sp.dCovStat);
            HIPCHK(hipMemcpyAsync(diag_stat, sp.dCovStat, sizeof diag_stat, hipMemcpyDeviceToHost, s));
        }
        if (jitter != 0.0) launch_add_diag(s, sp.dCovC, Mpad, M, jitter);
        HIPCHK(hipMemsetAsync(sp.dInfo, 0, sizeof(int) * 4, s));
        Members cov;   // one member: the posterior covariance, no RHS rows
        cov.A = sp.dCovC;
        cov.lda = Mpad;
        cov.invL = sp.dCovInv;
        cov.info = sp.dInfo;
        factor_buf(g, cov, mt, mt);
        HIPCHK(hipMemcpyAsync(&info, sp.dInfo, sizeof(int), hipMemcpyDeviceToHost, s));
        GP_SYNC(s);
        if (info == 0) break;
        // np.any(diagA <= 0.) raises before any jitter is tried (linalg.py:61-62)
        if (diag_stat[1] <= 0.0) return fail(GP_ERR_NOT_PD_DIAG, "not pd: non-positive diagonal elements");
        const int rcl = ladder_step(diag_stat[0] / (double)M, maxtries, info, &jitter, &tries);
        if (rcl == GP_ERR_NOT_PD_DIAG) return fail(rcl, "not pd: non-positive diagonal elements");
        if (rcl) {
            g_err = "not positive definite, even with jitter.";
            return rcl;
        }
    }
    launch_zero_upper_diag(s, sp.dCovC, Mpad, mt);
    // dev[s, m] = sum_{k <= m} z[s, k] C[m, k]: B = the factor's rows, the contraction ends at the diagonal tile
    GemmOpt o;
    o.k_end_tri = 1;
    gemm(g, s, 0, Dv, Mpad, Zd, Mpad, sp.dCovC, Mpad, 1, (int)Mpad, TileSet{0, st, 0, mt, 0}, o);
    if (mean && (rc = cov_mean_out(g, M, mean))) return rc;
    HIPCHK(hipMemcpy2DAsync(dev, sizeof(double) * M, Dv, sizeof(double) * Mpad, sizeof(double) * M, S, hipMemcpyDeviceToHost, s));
    GP_SYNC(s);
    if (jitter_used) *jitter_used = jitter;
    return 0;
}

// ---- the covariance against a resident second point set (csrc/sparse_cov.hip) ------------------------------------------------------
extern "C" int gp_sparse_cov_set_points(gp_t *g, const double *X2, int64_t R) {
    if (!g || !X2) return fail(GP_ERR_ARG, "null argument");
    GP_DEAD_CHECK(g);
    GP_NO_MEAN(g, "gp_sparse_cov_set_points");
    if (R < 1 || R > g->mc_max) return fail(GP_ERR_ARG, "R out of range (1..mc_max = %ld)", g->mc_max);
    if (!g->have_data) return fail(GP_ERR_STATE, "gp_set_data first");
    HIPCHK(hipSetDevice(g->device));
    GP_SYNC(g->s);
    SparseState &sp = g->sp;
    int rc;
    if ((rc = sp.dX2.reserve(R * g->D))) {
        sp.cR = 0;
        return rc;
    }
    HIPCHK(hipMemcpy(sp.dX2, X2, sizeof(double) * R * g->D, hipMemcpyHostToDevice));
    sp.cR = R;
    sp.g_valid = false;
    return 0;
}

// G = K(X2, Z) woodbury_inv, X2 / lengthscale and Z / lengthscale of the current fit: built by the first call after a fit or a new
// point set.  The product runs as 64 x 64 work units whatever R (the instance of sparse_posterior_rows): a row of G does not depend
// on the rows it is formed with.
static int cov_ensure_g(gp_ctx *g) {
    SparseState &sp = g->sp;
    const long n = sp.Mzpad, Mz = sp.Mz, R = sp.cR, Rpad = round_up(R, GP_TILE);
    hipStream_t s = g->s;
    int rc;
    if (!sp.zs_valid) {   // (as the fused rows path, api_sparse.hip)
        if ((rc = sp.dZs.reserve(Mz * g->D))) return rc;
        launch_sparse_scale_z(s, sp.dZ, Mz, g->kp, sp.dZs);
        sp.zs_valid = true;
    }
    if (sp.g_valid) return 0;
    if ((rc = sp.dCovA.reserve(Rpad * n))) return rc;
    if ((rc = sp.dG.reserve(Rpad * n))) return rc;
    if ((rc = sp.dX2s.reserve(R * g->D))) return rc;
    launch_cross_k(s, sp.dCovA, n, sp.dX2, R, Rpad, sp.dZ, Mz, n, g->kp);
    GemmOpt pinned;
    pinned.small = 1;
    // (woodbury_inv is symmetric: its rows serve as the B operand)
    launch_gemm_nt(s, 0, sp.dG, n, sp.dCovA, n, sp.dWinv, n, 1, (int)n, TileSet{0, (int)(Rpad / GP_TILE), 0, (int)(n / GP_TILE), 0}, pinned);
    launch_sparse_scale_z(s, sp.dX2, R, g->kp, sp.dX2s);
    sp.g_valid = true;
    return 0;
}

extern "C" int gp_sparse_cov_between(gp_t *g, const double *X1, int64_t M1, double *cov) {
    if (!g || !X1 || !cov) return fail(GP_ERR_ARG, "null argument");
    if (M1 < 1) return fail(GP_ERR_ARG, "M1 < 1");
    int rc;
    if ((rc = sparse_fitted(g))) return rc;
    SparseState &sp = g->sp;
    if (sp.cR < 1) return fail(GP_ERR_STATE, "gp_sparse_cov_set_points first");
    const long n = sp.Mzpad, Mz = sp.Mz, R = sp.cR;
    const int D = g->D;
    hipStream_t s = g->s;
    if (M1 <= ROWS_WIDE_M) {
        if ((rc = sp.covPin.reserve((long)ROWS_WIDE_M * R))) return rc;
        if ((rc = sp.cov_pass.ready(s))) return rc;
        if ((rc = cov_ensure_g(g))) return rc;
        return rows_passes(
            g, sp.cov_pass, X1, (int)M1, std::min((int)M1, ROWS_MAX_XS / D),
            [&](const RowsX &rx, const PassReport &r, unsigned *arrivals) {
                launch_sparse_cov_rows(s, sp.dG, n, Mz, R, sp.dX2s, rx, g->kp, sp.dZs, sp.covPin.p, r);
                arrivals[0] = sparse_cov_grid(R);
                return 0;
            },
            [&](int m0, int mc, const double *) { memcpy(cov + (long)m0 * R, sp.covPin.p, sizeof(double) * mc * R); });
    }
    if ((rc = sp.dCovX.reserve(M1 * D))) return rc;
    if ((rc = sp.dCovOut.reserve(M1 * R))) return rc;
    if ((rc = cov_ensure_g(g))) return rc;
    HIPCHK(hipMemcpyAsync(sp.dCovX, X1, sizeof(double) * M1 * D, hipMemcpyHostToDevice, s));
    launch_sparse_cov_table(s, sp.dG, n, Mz, R, sp.dX2s, sp.dCovX, M1, g->kp, sp.dZs, sp.dCovOut);
    HIPCHK(hipMemcpyAsync(cov, sp.dCovOut, sizeof(double) * M1 * R, hipMemcpyDeviceToHost, s));
    GP_SYNC(s);
    return 0;
}
