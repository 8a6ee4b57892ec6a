// Posterior paths (include/gphip.h, gp_paths_*): S samples of the posterior FUNCTION by pathwise conditioning on the resident
// factor -- a random-Fourier-feature draw from the prior plus an exact update through L (kernels: csrc/paths.hip).  gp_paths_set
// scales the caller's hyper-parameter-free draws from the resident parameters and solves for the update's weights V with the two
// substitutions alpha takes (solve_rows against the inverted diagonal panels, then launch_trsv_backward): nothing is factored, and
// the largest buffers are three blocks of at most 128 x Npad.  The paths belong to the factor: factor_results_dropped and
// factor_grown (api_internal.h) drop them.
#include "api_internal.h"

static_assert(GP_PATHS_MAX_S <= PATHS_MAX_SPAD && PATHS_MAX_SPAD <= GP_MAX_RHS, "the paths ride as right-hand-side rows of one tile");
static_assert(GP_PATHS_MAX_ROWS == PATHS_ROWS_M, "the kernel's argument takes GP_PATHS_MAX_ROWS locations");
static_assert(GP_PATHS_MAX_F % PATHS_MMA == 0, "whole feature tiles");
static_assert(PATHS_ROWS_M + ROWS_MAX_XS <= ROWS_OUT_DOUBLES, "values and gradients fit the pinned block");

// what every paths entry asks of the model (before anything is launched or changed)
static int paths_model(const gp_ctx *g, const char *who) {
    if (g->P != 1) return fail(GP_ERR_ARG, "%s needs P == 1", who);
    if (g->kp.gower) return fail(GP_ERR_ARG, "%s: a Gower kernel has no spectral density to draw frequencies from", who);
    GP_NO_MEAN(g, who);
    if (g->warp.n > 0) return fail(GP_ERR_STATE, "%s: not available while an output warp is on", who);
    return 0;
}
static int paths_resident(const gp_ctx *g, const char *who) {
    if (g->paths.S < 1) return fail(GP_ERR_STATE, "%s: no paths belong to the current fit (gp_paths_set after gp_fit)", who);
    return 0;
}
static int paths_normaliser(double y_mean, double y_std, const char *who) {
    if (!std::isfinite(y_mean)) return fail(GP_ERR_ARG, "%s: y_mean must be finite", who);
    if (!(y_std > 0.0) || !std::isfinite(y_std)) return fail(GP_ERR_ARG, "%s: y_std must be positive and finite", who);
    return 0;
}
static PathsPrior paths_prior(const gp_ctx *g) {
    const PathsState &p = g->paths;
    return PathsPrior{p.F, p.Fpad, p.Spad, p.amp, p.dOmega.p, p.dPhase.p, p.dWt.p};
}
static bool all_finite(const double *v, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

extern "C" int gp_paths_set(gp_t *g, int S, int F, const double *omega_unit, const double *phase, const double *w, const double *z_eps) {
    if (!g) return fail(GP_ERR_ARG, "null gp");
    GP_DEAD_CHECK(g);
    if (S < 0 || S > GP_PATHS_MAX_S) return fail(GP_ERR_ARG, "gp_paths_set: S out of range (0..%d)", GP_PATHS_MAX_S);
    if (S == 0) {   // clear
        g->paths.S = g->paths.F = 0;
        return 0;
    }
    GP_NO_LAPLACE(g, "gp_paths_set");   // (the update's residuals are y + eps - prior draw: targets, not labels)
    if (F < 1 || F > GP_PATHS_MAX_F) return fail(GP_ERR_ARG, "gp_paths_set: F out of range (1..%d)", GP_PATHS_MAX_F);
    if (!omega_unit || !phase || !w || !z_eps) return fail(GP_ERR_ARG, "null argument");
    GP_FITTED(g);
    int rc;
    if ((rc = paths_model(g, "gp_paths_set"))) return rc;
    const long N = g->N, Npad = g->Npad;
    const int D = g->D;
    if (!all_finite(omega_unit, (size_t)F * D) || !all_finite(phase, (size_t)F) || !all_finite(w, (size_t)S * F) ||
        !all_finite(z_eps, (size_t)S * N))
        return fail(GP_ERR_ARG, "gp_paths_set: a draw is not finite");
    PathsState &p = g->paths;
    const int Spad = (int)round_up(S, PATHS_MMA), Fpad = (int)round_up(F, PATHS_MMA);
    GP_SYNC(g->s);   // nothing on the stream still reads the paths that are about to go
    p.S = p.F = 0;
    if ((rc = ensure_panel_inv(g))) return rc;
    if ((rc = p.dOmega.reserve((long)GP_PATHS_MAX_F * D))) return rc;
    if ((rc = p.dPhase.reserve(GP_PATHS_MAX_F))) return rc;
    if ((rc = p.dWt.reserve((long)PATHS_MAX_SPAD * GP_PATHS_MAX_F))) return rc;
    if ((rc = p.dV.reserve((long)PATHS_MAX_SPAD * Npad))) return rc;
    if ((rc = p.dR.reserve((long)GP_TILE * Npad))) return rc;
    if ((rc = p.dZ.reserve((long)GP_TILE * Npad))) return rc;
    // the draws at the resident parameters: omega / lengthscale (one rounding each), a = sqrt(2 variance / F)
    std::vector<double> om((size_t)Fpad * D, 0.0), ph((size_t)Fpad, 0.0);
    for (int j = 0; j < F; ++j) {
        for (int d = 0; d < D; ++d) om[(size_t)j * D + d] = omega_unit[(size_t)j * D + d] / g->kp.ls[d];
        ph[j] = phase[j];
    }
    p.amp = std::sqrt(2.0 * g->kp.variance / (double)F);
    const double sd = std::sqrt(g->noise + 1e-8 + g->jitter);   // the diagonal of the factor (ky_diag + the ladder's jitter)
    hipStream_t s = g->s;
    HIPCHK(hipMemcpyAsync(p.dOmega, om.data(), sizeof(double) * om.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(p.dPhase, ph.data(), sizeof(double) * ph.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(p.dWt, 0, sizeof(double) * (size_t)Spad * Fpad, s));
    HIPCHK(hipMemcpy2DAsync(p.dWt, sizeof(double) * Fpad, w, sizeof(double) * F, sizeof(double) * F, S, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(p.dR, 0, sizeof(double) * (size_t)GP_TILE * Npad, s));
    HIPCHK(hipMemcpy2DAsync(p.dR, sizeof(double) * Npad, z_eps, sizeof(double) * N, sizeof(double) * N, S, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(p.dV, 0, sizeof(double) * (size_t)Spad * Npad, s));
    const PathsPrior pp{F, Fpad, Spad, p.amp, p.dOmega.p, p.dPhase.p, p.dWt.p};
    launch_paths_residual(s, pp, S, D, g->dX, g->dY, N, sd, p.dR, Npad);
    // V = L^-T (L^-1 r): the forward substitution as the candidate solve of one row tile (dR consumed, dZ = r L^-T), the
    // backward one as alpha's (dR is its workspace by then)
    Members m = ctx_members(g);
    m.T = p.dR;
    m.T2 = p.dZ;
    solve_rows(g, m, 1, 0);
    launch_trsv_backward(s, g->dA, Npad, g->dInvP, g->invp_W, Npad, p.dZ, Npad, S, p.dV, p.dR);
    GP_SYNC(s);   // the host copies above are the call's own: they go out of scope here
    p.S = S;
    p.F = F;
    p.Spad = Spad;
    p.Fpad = Fpad;
    return 0;
}

extern "C" int gp_paths_info(gp_t *g, int *S, int *F) {
    if (!g || !S || !F) return fail(GP_ERR_ARG, "null argument");
    *S = g->paths.S;
    *F = g->paths.S ? g->paths.F : 0;
    return 0;
}

// the table of every resident path over the resident candidates into paths.dTab [S, M], on the stream
static int paths_table(gp_ctx *g, double y_mean, double y_std, const char *who) {
    int rc;
    if ((rc = paths_model(g, who))) return rc;
    if ((rc = paths_resident(g, who))) return rc;
    if ((rc = paths_normaliser(y_mean, y_std, who))) return rc;
    PathsState &p = g->paths;
    if ((long)paths_table_lds_bytes(g->D, p.Spad) > g->lds_per_wg)
        return fail(GP_ERR_ARG, "%s: D = %d with %d paths needs %ld bytes of LDS per workgroup, the device gives %ld", who, g->D, p.S,
                    (long)paths_table_lds_bytes(g->D, p.Spad), g->lds_per_wg);
    if ((rc = p.dTab.reserve((long)p.S * g->M))) return rc;
    const long np = (long)paths_table_part_elems(g->M, g->N, p.S);
    if (np && (rc = p.dPart.reserve(np))) return rc;
    launch_paths_table(g->s, paths_prior(g), p.S, g->kp, g->dXs, g->M, g->dX, g->N, p.dV, g->Npad, y_mean, y_std, p.dTab,
                       np ? p.dPart.p : nullptr);
    return 0;
}

extern "C" int gp_paths_table(gp_t *g, double y_mean, double y_std, double *out) {
    if (!g || !out) return fail(GP_ERR_ARG, "null argument");
    GP_SCORING(g);
    int rc;
    if ((rc = paths_table(g, y_mean, y_std, "gp_paths_table"))) return rc;
    HIPCHK(hipMemcpyAsync(out, g->paths.dTab, sizeof(double) * (size_t)g->paths.S * g->M, hipMemcpyDeviceToHost, g->s));
    GP_SYNC(g->s);
    return 0;
}

extern "C" int gp_paths_argbest(gp_t *g, double y_mean, double y_std, int sense, int64_t *idx, double *val) {
    if (!g || !idx || !val) return fail(GP_ERR_ARG, "null argument");
    GP_SCORING(g);
    int rc;
    if ((rc = check_sense(sense))) return rc;
    if ((rc = paths_table(g, y_mean, y_std, "gp_paths_argbest"))) return rc;
    PathsState &p = g->paths;
    if ((rc = p.dRedV.reserve(paths_argbest_elems(GP_PATHS_MAX_S)))) return rc;
    if ((rc = p.dRedI.reserve(paths_argbest_elems(GP_PATHS_MAX_S)))) return rc;
    launch_paths_argbest(g->s, p.dTab, g->M, p.S, sense, p.dRedV, p.dRedI);
    long long hi[GP_PATHS_MAX_S];
    HIPCHK(hipMemcpyAsync(val, p.dRedV, sizeof(double) * p.S, hipMemcpyDeviceToHost, g->s));
    HIPCHK(hipMemcpyAsync(hi, p.dRedI, sizeof(long long) * p.S, hipMemcpyDeviceToHost, g->s));
    GP_SYNC(g->s);
    for (int s = 0; s < p.S; ++s) idx[s] = (int64_t)hi[s];
    return 0;
}

extern "C" int gp_paths_rows(gp_t *g, const double *Xs, int M, const int *path, double y_mean, double y_std, double *out, double *dout) {
    if (!g || !Xs || !path || !out) return fail(GP_ERR_ARG, "null argument");
    GP_FITTED(g);
    int rc;
    if ((rc = paths_model(g, "gp_paths_rows"))) return rc;
    if ((rc = paths_resident(g, "gp_paths_rows"))) return rc;
    if ((rc = paths_normaliser(y_mean, y_std, "gp_paths_rows"))) return rc;
    PathsState &p = g->paths;
    const int D = g->D;
    if (M < 1 || M > GP_PATHS_MAX_ROWS) return fail(GP_ERR_ARG, "gp_paths_rows: M out of range (1..%d)", GP_PATHS_MAX_ROWS);
    for (int m = 0; m < M; ++m)
        if (path[m] < 0 || path[m] >= p.S) return fail(GP_ERR_ARG, "gp_paths_rows: path[%d] = %d outside 0..%d", m, path[m], p.S - 1);
    if (!all_finite(Xs, (size_t)M * D)) return fail(GP_ERR_ARG, "gp_paths_rows: a location is not finite");
    const unsigned grid = paths_rows_grid(g->N, p.F);
    if ((rc = p.dRows.reserve((long)grid * PATHS_ROWS_GROW))) return rc;
    if ((rc = p.pass.ready(g->s))) return rc;
    const PathsPrior pp = paths_prior(g);
    // as every rows entry: as many locations per pass as M * D <= ROWS_MAX_XS coordinates allow (all of them up to D = 16, two at
    // D = 64), each pass with the path indices of its own locations.  A location's bits do not depend on its pass.
    const int width = std::min(M, ROWS_MAX_XS / D);
    int at = 0;   // first location of the pass being launched (rows_passes runs them in order, one at a time)
    return rows_passes(
        g, p.pass, Xs, M, width,
        [&](const RowsX &rx, const PassReport &r, unsigned *arrivals) {
            PathsPick pk{};
            for (int m = 0; m < rx.M; ++m) pk.path[m] = path[at + m];
            at += rx.M;
            launch_paths_rows(g->s, pp, rx, pk, g->kp, g->dX, g->N, p.dV, g->Npad, dout ? 1 : 0, y_mean, y_std, p.dRows, r);
            arrivals[0] = grid;
            return 0;
        },
        [&](int m0, int mc, const double *o) {
            memcpy(out + m0, o, sizeof(double) * mc);
            if (dout) memcpy(dout + (long)m0 * D, o + PATHS_ROWS_M, sizeof(double) * mc * D);
        });
}
