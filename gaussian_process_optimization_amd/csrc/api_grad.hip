// Hyper-parameter gradients of the LML, predictive gradients, acquisition gradients, dL_dK.
// Reference: Stationary.update_gradients_full (stationary.py:218-238), GP.predictive_gradients (gp.py:407-454).
#include "api_internal.h"

int lml_grad_lds_check(const gp_ctx *g, const char *who) {
    const size_t need = lml_grad_lds_bytes(g->D, g->kp.gower, g->P);
    if (need <= (size_t)g->lds_per_wg) return 0;
    return fail(GP_ERR_ARG, "%s: D = %d, P = %d, Gower %s need %zu bytes of LDS per workgroup in the gradient pass, the device has %ld",
                who, g->D, g->P, g->kp.gower ? "on" : "off", need, g->lds_per_wg);
}
int gradx_lds_check(const gp_ctx *g, const char *who) {
    const size_t need = gradx_lds_bytes(g->D, g->P);
    if (need <= (size_t)g->lds_per_wg) return 0;
    return fail(GP_ERR_ARG, "%s: D = %d, P = %d need %zu bytes of LDS per workgroup in the input-gradient pass, the device has %ld", who,
                g->D, g->P, need, g->lds_per_wg);
}

extern "C" int gp_lml_grad_lds(gp_t *g, int64_t *need, int64_t *available) {
    if (!g || !need || !available) return fail(GP_ERR_ARG, "null argument");
    GP_DEAD_CHECK(g);
    if (!g->have_data) return fail(GP_ERR_STATE, "gp_set_data first");
    *need = (int64_t)lml_grad_lds_bytes(g->D, g->kp.gower, g->P);
    *available = g->lds_per_wg;
    return 0;
}

// the fused dL_dK reduction for m's members: one pass per GP_GRAD_CH dimensions, its GP_GRAD_NACC sums side by side in SCAL_GRAD
void lml_grad_passes(gp_ctx *g, const Members &m) {
    int pass = 0;
    for (int d0 = 0; d0 < g->D; d0 += GP_GRAD_CH, ++pass) {
        launch_lml_grad(g->s, m.X, g->N, g->Npad, m.kp[0], g->ard, d0, m.alpha, g->P, m.Wi, g->Npad, m.partial,
                        m.scal + SCAL_GRAD.off + pass * GP_GRAD_NACC, m.nb, m.kpt, m.sV, m.sT, m.sT, m.sS, m.sX);
        if (!g->ard) break;
    }
}

// the gradients from those sums (h = the host copy of SCAL_GRAD)
void grads_from_sums(const double *h, const KernParams &kp, int ard, double *dvariance, double *dlengthscale, double *dnoise) {
    *dvariance = h[0] / kp.variance;  // stationary.py:224
    *dnoise = h[1];                   // gaussian.py:78-79
    if (ard) {
        for (int d = 0; d < kp.D; ++d)   // -sum tmp (dx_q)^2 / l_q^3, stationary.py:230-235,260-261
            dlengthscale[d] = -h[(d / GP_GRAD_CH) * GP_GRAD_NACC + 2 + (d % GP_GRAD_CH)] / kp.ls[d];
    } else {
        dlengthscale[0] = -h[2] / kp.ls[0];  // -sum(dL_dr * r) / l, stationary.py:237-238
    }
}

// dL/dX of the training inputs into dT behind the pass's own partials, as a phase (Ky^-1 is in dWi: ensure_wi ran, dT is free)
static int lml_grad_x_pass(gp_ctx *g, double **out) {
    const long np = gradx_partial_elems(g->Npad);
    int rc;
    if ((rc = g->dT.reserve(np + g->N * g->D))) return rc;   // (never grows after ensure_wi: Npad^2 covers it)
    const int ph = phase_begin(g, "lml_grad_x", 0.0, 8.0 * (double)g->N * g->N + 16.0 * (double)g->N * g->D);
    launch_gradx(g->s, g->dX, g->N, g->Npad, g->kp, g->dAlpha, g->P, g->dWi, g->Npad, g->dT, g->dT + np);
    phase_end(g, ph);
    *out = g->dT + np;
    return 0;
}

// dL_dX non-null: the input gradients behind the hyper-gradients, both handed over at the one synchronisation
int lml_grad_impl(gp_ctx *g, double *dvariance, double *dlengthscale, double *dnoise, bool reset_phases, double *dL_dX) {
    if (!g || !dvariance || !dlengthscale || !dnoise) return fail(GP_ERR_ARG, "null argument");
    GP_FITTED(g);
    GP_NO_LAPLACE(g, "gp_lml_grad");
    if (g->P > GP_GRAD_MAX_P) return fail(GP_ERR_ARG, "gp_lml_grad supports P <= %d", GP_GRAD_MAX_P);
    if (dL_dX && g->kp.gower) return fail(GP_ERR_ARG, "gp_lml_grad_x: not defined for a Gower model");
    int rc;
    if ((rc = lml_grad_lds_check(g, dL_dX ? "gp_fit_grad_x" : "gp_lml_grad"))) return rc;
    if (dL_dX && (rc = gradx_lds_check(g, "gp_fit_grad_x"))) return rc;
    // (a Gower model gets the fork's values: K through the Gower branch in the variance gradient, Euclidean dK/dr on the kernel's own
    // lengthscale in the lengthscale gradients, stationary.py:218-238 -- not derivatives of its LML, which the host layer knows)
    if (reset_phases) g->nphases = 0;
    if ((rc = ensure_wi(g))) return rc;
    // per-tile partials live in dT (free after ensure_wi): ntile * NACC doubles << Npad^2
    int ph = phase_begin(g, "lml_grad", 0.0, 8.0 * (double)g->N * g->N / 2);
    lml_grad_passes(g, ctx_members(g));
    phase_end(g, ph);
    const int npass = g->ard ? (g->D + GP_GRAD_CH - 1) / GP_GRAD_CH : 1;
    std::vector<double> host((size_t)GP_GRAD_NACC * npass);
    HIPCHK(hipMemcpyAsync(host.data(), g->dScal + SCAL_GRAD.off, sizeof(double) * host.size(), hipMemcpyDeviceToHost, g->s));
    if (dL_dX) {
        double *dev;
        if ((rc = lml_grad_x_pass(g, &dev))) return rc;
        HIPCHK(hipMemcpyAsync(dL_dX, dev, sizeof(double) * g->N * g->D, hipMemcpyDeviceToHost, g->s));
    }
    GP_SYNC(g->s);
    grads_from_sums(host.data(), g->kp, g->ard, dvariance, dlengthscale, dnoise);
    return 0;
}

extern "C" int gp_lml_grad(gp_t *g, double *dvariance, double *dlengthscale, double *dnoise) {
    return lml_grad_impl(g, dvariance, dlengthscale, dnoise, true);
}

// ---- dL/dX of the training inputs (InputWarpedGP.parameters_changed: kern.gradients_X(dL_dK, X), input_warped_gp.py:94-103) ----
extern "C" int gp_lml_grad_x(gp_t *g, double *dL_dX) {
    if (!g || !dL_dX) return fail(GP_ERR_ARG, "null argument");
    GP_FITTED(g);
    GP_NO_LAPLACE(g, "gp_lml_grad_x");
    GP_NO_MEAN(g, "gp_lml_grad_x");
    if (g->P > GP_GRAD_MAX_P) return fail(GP_ERR_ARG, "gp_lml_grad_x supports P <= %d", GP_GRAD_MAX_P);
    // the fork's Euclidean gradients_X on a Gower K is not a derivative of anything the warping could use
    if (g->kp.gower) return fail(GP_ERR_ARG, "gp_lml_grad_x: not defined for a Gower model");
    int rc;
    if ((rc = gradx_lds_check(g, "gp_lml_grad_x"))) return rc;
    g->nphases = 0;
    if ((rc = ensure_wi(g))) return rc;
    double *dev;
    if ((rc = lml_grad_x_pass(g, &dev))) return rc;
    HIPCHK(hipMemcpyAsync(dL_dX, dev, sizeof(double) * g->N * g->D, hipMemcpyDeviceToHost, g->s));
    GP_SYNC(g->s);
    return 0;
}

// gp_fit + gp_lml_grad as ONE call (what every L-BFGS evaluation of the hyper-parameter loop asks for:
// Model.objective_function + objective_function_gradients, core/model.py:96-127).  The first stages of the solve for
// L^-T ride behind the factorisation's latency-bound tail, like the candidate stages of gp_fit_predict.
// The fit of that call (shared with gp_fit_grad_x):
static int fit_grad_head(gp_ctx *g, int maxtries, double *lml, double *logdet, double *jitter_used) {
    HIPCHK(hipSetDevice(g->device));
    const int nt = (int)(g->Npad / GP_TILE);
    // emulated: Ky^-1 in residue form after the factorisation (wi_rns) instead of fp64 stages pipelined behind it
    const bool emu_wi = g->emulate_fp64 && g->emulate_fit && g->panel_tiles % 2 == 0;
    const bool can_pipe = g->lookahead && nt > g->panel_tiles && !emu_wi;
    int rc;
    if ((rc = fit_impl(g, maxtries, can_pipe ? Pipe::Identity : Pipe::None, 0))) return rc;
    if (lml) *lml = g->lml;
    if (logdet) *logdet = g->logdet;
    if (jitter_used) *jitter_used = g->jitter;
    return 0;
}
extern "C" int gp_fit_grad(gp_t *g, int maxtries, double *lml, double *logdet, double *jitter_used, double *dvariance,
                double *dlengthscale, double *dnoise) {
    if (!g || !dvariance || !dlengthscale || !dnoise) return fail(GP_ERR_ARG, "null argument");
    GP_DEAD_CHECK(g);
    if (!g->have_data || !g->have_params) return fail(GP_ERR_STATE, "set data and params before gp_fit_grad");
    if (g->P > GP_GRAD_MAX_P) return fail(GP_ERR_ARG, "gp_lml_grad supports P <= %d", GP_GRAD_MAX_P);
    int rc;
    if ((rc = lml_grad_lds_check(g, "gp_fit_grad"))) return rc;   // before the factorisation: a refused call leaves the fit as it was
    if ((rc = fit_grad_head(g, maxtries, lml, logdet, jitter_used))) return rc;
    return lml_grad_impl(g, dvariance, dlengthscale, dnoise, false);
}

// gp_fit_grad followed by the input-gradient pass, as ONE call with one final hand-over: what every L-BFGS evaluation of the
// input-warped model asks for (the warped inputs changed, so the fit is new each time)
extern "C" int gp_fit_grad_x(gp_t *g, int maxtries, double *lml, double *logdet, double *jitter_used, double *dvariance,
                             double *dlengthscale, double *dnoise, double *dL_dX) {
    if (!g || !dvariance || !dlengthscale || !dnoise || !dL_dX) return fail(GP_ERR_ARG, "null argument");
    GP_DEAD_CHECK(g);
    if (!g->have_data || !g->have_params) return fail(GP_ERR_STATE, "set data and params before gp_fit_grad_x");
    GP_NO_MEAN(g, "gp_fit_grad_x");
    if (g->P > GP_GRAD_MAX_P) return fail(GP_ERR_ARG, "gp_lml_grad_x supports P <= %d", GP_GRAD_MAX_P);
    if (g->kp.gower) return fail(GP_ERR_ARG, "gp_lml_grad_x: not defined for a Gower model");
    int rc;
    if ((rc = lml_grad_lds_check(g, "gp_fit_grad_x"))) return rc;
    if ((rc = gradx_lds_check(g, "gp_fit_grad_x"))) return rc;
    if ((rc = fit_grad_head(g, maxtries, lml, logdet, jitter_used))) return rc;
    return lml_grad_impl(g, dvariance, dlengthscale, dnoise, false, dL_dX);
}

// ---- second candidate-sized buffer (beta = K(Xs,X) Ky^-1, or the full covariance) -----------------
int ensure_grad_buffers(gp_ctx *g, long elemsBeta, long M) {
    int rc;
    if ((rc = g->dCov.reserve(elemsBeta))) return rc;
    const long need = M * (long)g->D * std::max(1, g->P);
    if (g->dDacq.cap >= need) return 0;   // the last of the three to be allocated: all are there, at one capacity
    for (DevBuf<double> *b : {&g->dDm, &g->dDv, &g->dDacq}) b->release();
    if ((rc = g->dDm.reserve(need))) return rc;
    if ((rc = g->dDv.reserve(need))) return rc;
    return g->dDacq.reserve(need);
}

// predictive gradients of all resident candidates into dDm [M, D, P] and dDv [M, D]
// A Gower model (gp_set_gower) gets what the fork computes for it (gp.py:407-454 over stationary.py:336-364): K(Xs, X) -- and
// with it beta -- takes the Gower branch (stationary.py:116-135), while gradients_X stays the Euclidean formula on the
// kernel's own lengthscale parameter (_inv_dist :251-258, dK_dr_via_X :142-148).  kp.ls holds that parameter, kp.gdiv the
// ranges: cross_k reads the latter, predict_grad_kernel the former.  Inconsistent as a derivative, but it is the function
// the reference's L-BFGS (run.py:1206-1225) and estimate_L (run.py:1244) see.
int run_predict_grad(gp_ctx *g) {
    int rc;
    if (g->M <= g->small_m && !g->wi_valid) {
        // A handful of locations right after a fit: beta = Ky^-1 k* by TWO substitutions against L (dpotrs, the reference's own route
        // for alpha, exact_gaussian_inference.py:60) instead of building Ky^-1 first -- the potri-equivalent costs 2 N^3 / 3 (50 ms at
        // N = 16384), ~90 short launches cost 1.4 ms.  Posterior mean / variance of the same rows fall out on the way.
        const long M = g->M, N = g->N, Npad = g->Npad;
        if ((rc = ensure_panel_inv(g))) return rc;
        if ((rc = ensure_out(g))) return rc;
        if ((rc = g->dT.reserve((long)GP_TILE * Npad))) return rc;
        if ((rc = g->dT2.reserve((long)GP_TILE * Npad))) return rc;
        if ((rc = ensure_grad_buffers(g, (long)GP_TILE * Npad, M))) return rc;
        g->w_in_t2 = false;
        launch_cross_k_rows(g->s, g->dT, Npad, g->dXs, (int)M, g->dX, N, Npad, g->kp);
        launch_small_forward_solve(g->s, g->dA, Npad, g->dInvP, g->invp_W, Npad, g->dT, g->dT2, Npad, (int)M);   // dT2 = w rows
        launch_predict_reduce(g->s, g->dT2, Npad, M, N, g->dA + Npad * Npad, Npad, g->P, g->kp.variance, g->noise, g->dMean,
                              g->dVar);
        mean_add(g, g->dXs, M, g->dMean);
        g->predicted = true;       // GPModel.predict: with_noise=True (gpmodel.py:102)
        g->predicted_noise = 1;
        launch_trsv_backward(g->s, g->dA, Npad, g->dInvP, g->invp_W, Npad, g->dT2, Npad, (int)M, g->dCov, g->dT);   // beta = L^-T w
        launch_predict_grad(g->s, g->dXs, M, g->dX, N, g->kp, g->dAlpha, Npad, g->P, g->dCov, Npad, g->dDm, g->dDv);
        mean_add_grad(g, M, g->dDm);
        return 0;
    }
    if ((rc = ensure_wi(g))) return rc;
    const long M = g->M, N = g->N, Npad = g->Npad;
    const int nt = (int)(Npad / GP_TILE);
    const long mc_max = std::min(g->mc_max, round_up(M, GP_TILE));
    if ((rc = g->dT.reserve(mc_max * Npad))) return rc;
    if ((rc = ensure_grad_buffers(g, mc_max * Npad, M))) return rc;
    for (long m0 = 0; m0 < M; m0 += mc_max) {
        const long mc = std::min(mc_max, M - m0);
        const long mcpad = round_up(mc, GP_TILE);
        const int mt = (int)(mcpad / GP_TILE);
        if (M <= g->small_m)
            launch_cross_k_rows(g->s, g->dT, Npad, g->dXs, (int)M, g->dX, N, Npad, g->kp);
        else
            launch_cross_k(g->s, g->dT, Npad, g->dXs + m0 * g->D, mc, mcpad, g->dX, N, Npad, g->kp);
        // beta = K(Xs, X) Ky^-1   (gp.py:451-452; Ky^-1 symmetric => rows of Wi serve as the B operand)
        if (M <= g->small_m)   // a handful of rows: row dots with Ky^-1, one read of it (smallm.hip)
            launch_small_wi_product(g->s, g->dWi, Npad, Npad, g->dT, Npad, (int)mc, g->dCov, Npad);
        else
            gemm(g, g->s, 0, g->dCov, Npad, g->dT, Npad, g->dWi, Npad, 1, (int)Npad, TileSet{0, mt, 0, nt, 0});
        launch_predict_grad(g->s, g->dXs + m0 * g->D, mc, g->dX, N, g->kp, g->dAlpha, Npad, g->P, g->dCov, Npad,
                            g->dDm + m0 * g->D * g->P, g->dDv + m0 * g->D);
    }
    mean_add_grad(g, M, g->dDm);   // a resident mean function: dmdx[m, d, p] += A[d, p]
    g->predicted = false;  // dT no longer holds the solved candidates
    return 0;
}

// dDm [M, D, P] (and dDv [M, D]) to the caller, drained
static int grads_out(gp_ctx *g, double *dmdx, double *dvdx) {
    HIPCHK(hipMemcpyAsync(dmdx, g->dDm, sizeof(double) * g->M * g->D * g->P, hipMemcpyDeviceToHost, g->s));
    if (dvdx) HIPCHK(hipMemcpyAsync(dvdx, g->dDv, sizeof(double) * g->M * g->D, hipMemcpyDeviceToHost, g->s));
    GP_SYNC(g->s);
    return 0;
}

extern "C" int gp_predict_grad(gp_t *g, double *dmdx, double *dvdx) {
    if (!g || !dmdx) return fail(GP_ERR_ARG, "null argument");
    GP_SCORING(g);
    int rc;
    if (!dvdx) {
        // the mean's gradients alone (what estimate_L maximises, batch_local_penalization.py:55-58): gradients_X(alpha^T, X*, X) needs
        // neither Ky^-1 nor K(X*, X) Ky^-1 -- one pass of O(M N D) instead of 2 N^3 / 3 + N^2 M flops
        if ((rc = ensure_grad_buffers(g, 1, g->M))) return rc;
        launch_predict_grad(g->s, g->dXs, g->M, g->dX, g->N, g->kp, g->dAlpha, g->Npad, g->P, nullptr, 0, g->dDm, g->dDv);
        mean_add_grad(g, g->M, g->dDm);
    } else if ((rc = run_predict_grad(g))) {
        return rc;
    }
    return grads_out(g, dmdx, dvdx);
}

// The negated acquisition of the resident candidates -- penalised when lp is given -- to out [M] and, when dout is given, its
// x-gradient to dout [M, D], drained (AcquisitionLP.acquisition_function_withGradients, GPyOpt/GPyOpt/acquisitions/LP.py:112-140).
int acq_values(gp_ctx *g, const AcqSpec &a, const LpSpec *lp, double *out, double *dout) {
    int rc;
    if ((rc = run_acq(g, a, lp, dout != nullptr))) return rc;
    return scores_out(g, g->dAcq, g->dDacq, g->M, g->D, out, dout);
}

extern "C" int gp_acq_grad(gp_t *g, int type, double par, double fmin, double y_mean, double y_std, double *out, double *dout) {
    if (!g || !out || !dout) return fail(GP_ERR_ARG, "null argument");
    GP_SCORING(g);
    return acq_values(g, exact_spec(g, AcqSpec{type, par, fmin, y_mean, y_std}), nullptr, out, dout);
}

extern "C" int gp_acq_lp_grad(gp_t *g, int type, double par, double fmin, double y_mean, double y_std, int transform,
                              const double *Xb, int nb, const double *r_x0, const double *s_x0, double *out, double *dout) {
    if (!g || !out || !dout) return fail(GP_ERR_ARG, "null argument");
    GP_SCORING(g);
    const LpSpec lp{transform, Xb, nb, r_x0, s_x0};
    return acq_values(g, exact_spec(g, AcqSpec{type, par, fmin, y_mean, y_std}), &lp, out, dout);
}

// ---- dL_dK = 0.5 (alpha alpha^T - P Ky^-1)  (exact_gaussian_inference.py:70) -------------------------------
// What grad_dict['dL_dK'] carries into kern.update_gradients_full (gp.py:269) when the reference's own kernel classes
// consume it on the host.  gp_lml_grad forms the same matrix implicitly inside its fused reduction.
extern "C" int gp_get_dl_dk(gp_t *g, double *dL_dK) {
    if (!g || !dL_dK) return fail(GP_ERR_ARG, "null argument");
    GP_FITTED(g);
    GP_NO_LAPLACE(g, "gp_get_dl_dk");
    int rc;
    if ((rc = ensure_wi(g))) return rc;  // leaves dT free (Npad x Npad)
    const long N = g->N, Npad = g->Npad;
    launch_dldk(g->s, g->dT, Npad, g->dAlpha, Npad, g->P, g->dWi, Npad, N);
    GP_SYNC(g->s);
    HIPCHK(hipMemcpy2D(dL_dK, sizeof(double) * N, g->dT, sizeof(double) * Npad, sizeof(double) * N, N,
                       hipMemcpyDeviceToHost));
    g->predicted = false;  // dT was reused
    return 0;
}
