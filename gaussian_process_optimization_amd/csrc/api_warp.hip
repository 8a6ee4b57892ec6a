// The output-warped GP (GPy.models.WarpedGP, GPy/GPy/models/warped_gp.py:13-160 over TanhFunction,
// GPy/GPy/util/warping_functions.py:71-169): the warp of the resident targets, its LML gradient, and predictions pushed back
// through the inverse.  The GP itself is the unchanged fit on f(Y); see include/gphip.h for the contract of each entry point.
#include "api_internal.h"

// dY <- f(dYraw), warp_logjac <- sum log f'; raw_in_dY: dY still holds the raw targets (a new upload, or no warp was on), which
// go to dYraw first.  Enqueued; the caller drains.
int warp_apply(gp_ctx *g, bool raw_in_dY) {
    if (raw_in_dY) {
        int rc;
        if ((rc = g->dYraw.reserve(g->capN))) return rc;
        HIPCHK(hipMemcpyAsync(g->dYraw, g->dY, sizeof(double) * g->N, hipMemcpyDeviceToDevice, g->s));
    }
    launch_warp_y(g->s, g->dYraw, g->N, g->warp, g->dY, g->dScal + SCAL_WARP_LOGJAC.off);
    HIPCHK(hipMemcpyAsync(&g->warp_logjac, g->dScal + SCAL_WARP_LOGJAC.off, sizeof(double), hipMemcpyDeviceToHost, g->s));
    return 0;
}

static int warp_from_args(int n_terms, const double *psi, double d, WarpParams *w) {
    if (n_terms < 0 || n_terms > GP_WARP_MAX_TERMS)
        return fail(GP_ERR_ARG, "n_terms out of range (0..%d)", GP_WARP_MAX_TERMS);
    memset(w, 0, sizeof *w);
    w->d = 1.0;
    if (n_terms == 0) return 0;
    if (!psi) return fail(GP_ERR_ARG, "null argument");
    w->n = n_terms;
    w->d = d;
    for (int i = 0; i < n_terms; ++i) {
        w->a[i] = psi[3 * i];
        w->b[i] = psi[3 * i + 1];
        w->c[i] = psi[3 * i + 2];
    }
    if (!warp_params_valid(*w)) return fail(GP_ERR_ARG, "warp parameters must be finite with a >= 0, b >= 0 and d > 0");
    return 0;
}

extern "C" int gp_set_output_warp(gp_t *g, int n_terms, const double *psi, double d, double *log_jacobian) {
    if (!g) return fail(GP_ERR_ARG, "null gp");
    GP_DEAD_CHECK(g);
    WarpParams w;
    int rc;
    if ((rc = warp_from_args(n_terms, psi, d, &w))) return rc;
    GP_NO_MEAN(g, "gp_set_output_warp");
    if (!g->have_data) return fail(GP_ERR_STATE, "gp_set_data first");
    if (w.n > 0 && g->P != 1) return fail(GP_ERR_STATE, "an output warp takes P = 1 (the data has P = %d)", g->P);
    HIPCHK(hipSetDevice(g->device));
    if (w.n == 0) {
        if (g->warp.n > 0) {   // off: the raw targets again
            HIPCHK(hipMemcpyAsync(g->dY, g->dYraw, sizeof(double) * g->N, hipMemcpyDeviceToDevice, g->s));
            GP_SYNC(g->s);
            g->warp = w;
            g->warp_logjac = 0.0;
            fit_dropped(g);
            sparse_fit_dropped(g);
        }
        if (log_jacobian) *log_jacobian = 0.0;
        return 0;
    }
    const bool was_off = g->warp.n == 0;   // (a warp that is on already left the raw targets in dYraw)
    g->warp = w;
    if ((rc = warp_apply(g, was_off))) {
        if (was_off) g->warp.n = 0;
        return rc;
    }
    fit_dropped(g);
    sparse_fit_dropped(g);
    GP_SYNC(g->s);
    if (log_jacobian) *log_jacobian = g->warp_logjac;
    return 0;
}

extern "C" int gp_get_targets(gp_t *g, double *Y) {
    if (!g || !Y) return fail(GP_ERR_ARG, "null argument");
    GP_DEAD_CHECK(g);
    if (!g->have_data) return fail(GP_ERR_STATE, "gp_set_data first");
    HIPCHK(hipSetDevice(g->device));
    HIPCHK(hipMemcpyAsync(Y, g->dY, sizeof(double) * g->N * g->P, hipMemcpyDeviceToHost, g->s));
    GP_SYNC(g->s);
    return 0;
}

extern "C" int gp_warp_grad(gp_t *g, double *dpsi, double *dd) {
    if (!g || !dpsi || !dd) return fail(GP_ERR_ARG, "null argument");
    GP_FITTED(g);
    GP_NO_MEAN(g, "gp_warp_grad");
    if (g->warp.n < 1) return fail(GP_ERR_STATE, "gp_set_output_warp first");
    const int np = 3 * g->warp.n + 1;
    double host[GP_WARP_NPSI];
    launch_warp_grad(g->s, g->dYraw, g->dAlpha, g->N, g->warp, g->dScal + SCAL_WARP_GRAD.off);
    HIPCHK(hipMemcpyAsync(host, g->dScal + SCAL_WARP_GRAD.off, sizeof(double) * np, hipMemcpyDeviceToHost, g->s));
    GP_SYNC(g->s);
    for (int q = 0; q < np - 1; ++q) dpsi[q] = host[q];
    *dd = host[np - 1];
    return 0;
}

// gp_set_output_warp, gp_fit_grad and gp_warp_grad in sequence: the same launches, hence the same bits
extern "C" int gp_fit_grad_warp(gp_t *g, int n_terms, const double *psi, double d, int maxtries, double *lml, double *logdet,
                                double *jitter_used, double *dvariance, double *dlengthscale, double *dnoise, double *log_jacobian,
                                double *dpsi, double *dd) {
    if (!g || !psi || !dvariance || !dlengthscale || !dnoise || !dpsi || !dd) return fail(GP_ERR_ARG, "null argument");
    if (n_terms < 1) return fail(GP_ERR_ARG, "gp_fit_grad_warp takes a warp of 1..%d terms", GP_WARP_MAX_TERMS);
    GP_NO_MEAN(g, "gp_fit_grad_warp");
    int rc;
    // gp_fit_grad's refusal of a shape whose gradient pass does not fit the LDS, before the warp changes the targets
    if (!g->dead && g->have_data && (rc = lml_grad_lds_check(g, "gp_fit_grad_warp"))) return rc;
    if ((rc = gp_set_output_warp(g, n_terms, psi, d, log_jacobian))) return rc;
    if ((rc = gp_fit_grad(g, maxtries, lml, logdet, jitter_used, dvariance, dlengthscale, dnoise))) return rc;
    return gp_warp_grad(g, dpsi, dd);
}

static int nodes_from_args(int deg, const double *nodes, const double *weights, WarpNodes *gh) {
    if (!nodes || !weights) return fail(GP_ERR_ARG, "null argument");
    if (deg < 1 || deg > GP_WARP_MAX_DEG) return fail(GP_ERR_ARG, "deg out of range (1..%d)", GP_WARP_MAX_DEG);
    memset(gh, 0, sizeof *gh);
    gh->deg = deg;
    for (int k = 0; k < deg; ++k) {
        gh->t[k] = nodes[k];
        gh->w[k] = weights[k];
    }
    return 0;
}

// the moments of M Gaussians (device pointers) into the tail of dWarp, then to the caller, drained
static int moments_out(gp_ctx *g, const double *dmean, const double *dvar, long M, double y_mean, double y_std, const WarpNodes &gh,
                       double *mean, double *var, double *median, double *partials) {
    double *wm = g->dWarp + 2 * M, *wv = wm + M, *md = wv + M, *pt = md + M;
    launch_warp_moments(g->s, dmean, dvar, M, y_mean, y_std, g->warp, gh, wm, wv, median ? md : nullptr, partials ? pt : nullptr);
    HIPCHK(hipMemcpyAsync(mean, wm, sizeof(double) * M, hipMemcpyDeviceToHost, g->s));
    HIPCHK(hipMemcpyAsync(var, wv, sizeof(double) * M, hipMemcpyDeviceToHost, g->s));
    if (median) HIPCHK(hipMemcpyAsync(median, md, sizeof(double) * M, hipMemcpyDeviceToHost, g->s));
    if (partials) HIPCHK(hipMemcpyAsync(partials, pt, sizeof(double) * 4 * M, hipMemcpyDeviceToHost, g->s));
    GP_SYNC(g->s);
    return 0;
}

extern "C" int gp_predict_warped(gp_t *g, int include_noise, double y_mean, double y_std, int deg, const double *nodes,
                                 const double *weights, int want_median, double *mean, double *var, double *median,
                                 double *partials) {
    if (!g || !mean || !var || (want_median && !median)) return fail(GP_ERR_ARG, "null argument");
    GP_SCORING(g);
    GP_NO_MEAN(g, "gp_predict_warped");
    if (g->P != 1) return fail(GP_ERR_STATE, "gp_predict_warped needs P == 1");
    WarpNodes gh;
    int rc;
    if ((rc = nodes_from_args(deg, nodes, weights, &gh))) return rc;
    if ((rc = ensure_out(g))) return rc;
    if (!g->predicted || g->predicted_noise != (include_noise ? 1 : 0))
        if ((rc = run_predict(g, include_noise))) return rc;
    if ((rc = g->dWarp.reserve(9 * g->M))) return rc;
    return moments_out(g, g->dMean, g->dVar, g->M, y_mean, y_std, gh, mean, var, want_median ? median : nullptr, partials);
}

extern "C" int gp_warp_moments(gp_t *g, const double *mean_in, const double *var_in, int64_t M, double y_mean, double y_std, int deg,
                               const double *nodes, const double *weights, int want_median, double *mean, double *var,
                               double *median, double *partials) {
    if (!g || !mean_in || !var_in || !mean || !var || (want_median && !median)) return fail(GP_ERR_ARG, "null argument");
    GP_DEAD_CHECK(g);
    if (M < 1) return fail(GP_ERR_ARG, "M < 1");
    WarpNodes gh;
    int rc;
    if ((rc = nodes_from_args(deg, nodes, weights, &gh))) return rc;
    HIPCHK(hipSetDevice(g->device));
    if ((rc = g->dWarp.reserve(9 * M))) return rc;
    HIPCHK(hipMemcpyAsync(g->dWarp, mean_in, sizeof(double) * M, hipMemcpyHostToDevice, g->s));
    HIPCHK(hipMemcpyAsync(g->dWarp + M, var_in, sizeof(double) * M, hipMemcpyHostToDevice, g->s));
    return moments_out(g, g->dWarp, g->dWarp + M, M, y_mean, y_std, gh, mean, var, want_median ? median : nullptr, partials);
}

extern "C" int gp_warp_inverse(gp_t *g, const double *z, int64_t n, double *y) {
    if (!g || !z || !y) return fail(GP_ERR_ARG, "null argument");
    GP_DEAD_CHECK(g);
    if (n < 1) return fail(GP_ERR_ARG, "n < 1");
    HIPCHK(hipSetDevice(g->device));
    int rc;
    if ((rc = g->dWarp.reserve(2 * n))) return rc;
    HIPCHK(hipMemcpyAsync(g->dWarp, z, sizeof(double) * n, hipMemcpyHostToDevice, g->s));
    launch_warp_inverse(g->s, g->dWarp, n, g->warp, g->dWarp + n);
    HIPCHK(hipMemcpyAsync(y, g->dWarp + n, sizeof(double) * n, hipMemcpyDeviceToHost, g->s));
    GP_SYNC(g->s);
    return 0;
}
