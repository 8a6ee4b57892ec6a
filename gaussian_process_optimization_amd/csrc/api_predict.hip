// Candidates: posterior mean / variance, acquisitions, arg-best / top-k, local penalisation, full covariance and
// posterior samples.  Reference: PosteriorExact._raw_predict (posterior.py:273-302), GPyOpt acquisitions/{EI,LCB,MPI,LP}.py.
#include "api_internal.h"

// ---- candidates / predict -----------------------------------------------------------------------
extern "C" int gp_set_candidates(gp_t *g, const double *Xs, int64_t M) {
    if (!g || !Xs) return fail(GP_ERR_ARG, "null argument");
    GP_DEAD_CHECK(g);
    if (!g->have_data) return fail(GP_ERR_STATE, "gp_set_data first");
    if (M < 1) return fail(GP_ERR_ARG, "M < 1");
    HIPCHK(hipSetDevice(g->device));
    GP_SYNC(g->s);
    int rc;
    if ((rc = g->dXs.reserve((long)M * g->D))) return rc;
    HIPCHK(hipMemcpy(g->dXs, Xs, sizeof(double) * M * g->D, hipMemcpyHostToDevice));
    g->M = M;
    g->predicted = false;
    if (g->cost_tab == 1) g->cost_tab = 0;
    g->feas.K = 0;   // the cached probability of feasibility was this table's
    return 0;
}

// gp_set_candidates of the Kumaraswamy-warped table (KumarWarping.f, input_warping_functions.py:179-200), warped on the device
extern "C" int gp_set_candidates_kumar(gp_t *g, const double *Xs, int64_t M, const int *warp, const double *a, const double *b,
                                       const double *xmin, const double *xmax, double *warped_out) {
    if (!g || !Xs || !warp || !a || !b || !xmin || !xmax) return fail(GP_ERR_ARG, "null argument");
    GP_DEAD_CHECK(g);
    if (!g->have_data) return fail(GP_ERR_STATE, "gp_set_data first");
    GP_NO_MEAN(g, "gp_set_candidates_kumar");
    for (int q = 0; q < g->D; ++q) {
        if (!warp[q]) continue;
        if (!(a[q] > 0.0) || !(b[q] > 0.0) || !std::isfinite(a[q]) || !std::isfinite(b[q]))
            return fail(GP_ERR_ARG, "gp_set_candidates_kumar: a, b must be positive and finite (dimension %d)", q);
        if (!(xmax[q] > xmin[q]) || !std::isfinite(xmax[q]) || !std::isfinite(xmin[q]))
            return fail(GP_ERR_ARG, "gp_set_candidates_kumar: xmax <= xmin (dimension %d)", q);
    }
    int rc;
    if ((rc = gp_set_candidates(g, Xs, M))) return rc;
    const long mc_max = std::min(g->mc_max, round_up(M, GP_TILE));   // the chunks of run_predict
    for (long m0 = 0; m0 < M; m0 += mc_max)
        launch_kumar_warp(g->s, g->dXs, m0, std::min(mc_max, (long)M - m0), g->D, warp, a, b, xmin, xmax);
    if (warped_out) HIPCHK(hipMemcpyAsync(warped_out, g->dXs, sizeof(double) * M * g->D, hipMemcpyDeviceToHost, g->s));
    GP_SYNC(g->s);
    return 0;
}

int run_predict(gp_ctx *g, int include_noise, bool tiles_only, const ChunkHook *chunk) {
    if (!g->fitted) return fail(GP_ERR_STATE, "gp_fit first");
    if (g->M < 1) return fail(GP_ERR_STATE, "gp_set_candidates first");
    HIPCHK(hipSetDevice(g->device));
    const long M = g->M, N = g->N, Npad = g->Npad;
    const int P = g->P;
    int rc;
    g->nphases = 0;
    const long mc_max = std::min(g->mc_max, round_up(M, GP_TILE));
    if ((rc = ensure_panel_inv(g))) return rc;
    if ((rc = g->dT.reserve(mc_max * Npad))) return rc;
    if ((rc = g->dT2.reserve(mc_max * Npad))) return rc;
    g->w_in_t2 = false;   // dT2 takes the solved candidate rows
    if (M <= g->small_m && !tiles_only) {
        // A handful of rows (the acquisition optimiser's one-row calls): the solve as matrix-vector work bound by ONE read of
        // L (smallm.hip) instead of ~45 dependent tile launches; always true fp64.
        int ph = phase_begin(g, "cross_k", 0.0, 8.0 * (double)(N + M) * g->D + 8.0 * (double)N * M);
        launch_cross_k_rows(g->s, g->dT, Npad, g->dXs, (int)M, g->dX, g->N, Npad, g->kp);
        phase_end(g, ph);
        ph = phase_begin(g, "cand_solve_rows", (double)N * N * M, 8.0 * (double)N * N / 2);
        launch_small_forward_solve(g->s, g->dA, Npad, g->dInvP, g->invp_W, Npad, g->dT, g->dT2, Npad, (int)M);
        phase_end(g, ph);
        ph = phase_begin(g, "reduce", 0.0, 8.0 * (double)N * M);
        launch_predict_reduce(g->s, g->dT2, Npad, M, N, g->dA + Npad * Npad, Npad, P, g->kp.variance,
                              include_noise ? g->noise : 0.0, g->dMean, g->dVar);
        mean_add(g, g->dXs, M, g->dMean);   // a resident mean function: m(x*) joins the mean upstream of every cache and score
        phase_end(g, ph);
        g->predicted = true;
        g->predicted_noise = include_noise ? 1 : 0;
        return 0;
    }
    for (long m0 = 0; m0 < M; m0 += mc_max) {
        const long mc = std::min(mc_max, M - m0);
        const long mcpad = round_up(mc, GP_TILE);
        int ph = phase_begin(g, "cross_k", 0.0, 8.0 * (double)(N + mc) * g->D + 8.0 * (double)N * mc);
        launch_cross_k(g->s, g->dT, Npad, g->dXs + m0 * g->D, mc, mcpad, g->dX, g->N, Npad, g->kp);
        phase_end(g, ph);
        ph = phase_begin(g, g->emulate_fp64 ? "cand_solve_emulated" : "cand_solve", (double)N * N * mc, 0.0);
        if (g->emulate_fp64 && !g->lap.on) {   // (a Laplace-fitted context: true fp64, its factor has no fixed-point bound)
            rc = solve_rows_rns(g, g->dT, g->dT2, (int)(mcpad / GP_TILE));
            if (rc == GP_ERR_RANGE) {   // non-finite candidates / factor: this chunk again in true fp64 (NaNs propagate as in the reference)
                ++g->emu_fallbacks;
                launch_cross_k(g->s, g->dT, Npad, g->dXs + m0 * g->D, mc, mcpad, g->dX, g->N, Npad, g->kp);
                solve_rows(g, ctx_members(g), (int)(mcpad / GP_TILE), 0);
            } else if (rc) {
                return rc;
            }
        } else {
            solve_rows(g, ctx_members(g), (int)(mcpad / GP_TILE), 0);
        }
        phase_end(g, ph);
        ph = phase_begin(g, "reduce", 0.0, 8.0 * (double)N * mc);
        launch_predict_reduce(g->s, g->dT2, Npad, mc, N, g->dA + Npad * Npad, Npad, P, g->kp.variance,
                              include_noise ? g->noise : 0.0, g->dMean + m0 * P, g->dVar + m0);
        mean_add(g, g->dXs + m0 * g->D, mc, g->dMean + m0 * P);
        phase_end(g, ph);
        if (chunk && (rc = (*chunk)(m0, mc, mcpad))) return rc;
    }
    g->predicted = true;
    g->predicted_noise = include_noise ? 1 : 0;
    return 0;
}

int ensure_out(gp_ctx *g) {
    const long need = g->M * (long)std::max(1, g->P);
    if (g->dAcq.cap >= need) return 0;   // the last of the three to be allocated: all are there, at one capacity
    for (DevBuf<double> *b : {&g->dMean, &g->dVar, &g->dAcq}) b->release();
    int rc;
    if ((rc = g->dMean.reserve(need))) return rc;
    if ((rc = g->dVar.reserve(need))) return rc;
    return g->dAcq.reserve(need);
}

extern "C" int gp_predict(gp_t *g, int include_noise, double *mean, double *var) {
    if (!g) return fail(GP_ERR_ARG, "null gp");
    GP_SCORING(g);
    int rc;
    if ((rc = ensure_out(g))) return rc;
    if ((rc = run_predict(g, include_noise))) return rc;
    if (mean) HIPCHK(hipMemcpyAsync(mean, g->dMean, sizeof(double) * g->M * g->P, hipMemcpyDeviceToHost, g->s));
    if (var) HIPCHK(hipMemcpyAsync(var, g->dVar, sizeof(double) * g->M, hipMemcpyDeviceToHost, g->s));
    GP_SYNC(g->s);
    return 0;
}

// ---- the checks of what a caller asks to have scored, one each --------------------------------------------------------------
int check_acq(const gp_ctx *g, const AcqSpec &a, const LpSpec *lp) {
    if (g->P != 1) return fail(GP_ERR_ARG, "acquisitions need P == 1");
    const int base = acq_rule(a);
    const bool feas = acq_times_feas(a);
    if (base == GP_ACQ_MES && a.mes_ok) GP_NO_LAPLACE(g, "GP_ACQ_MES");
    if (base == GP_ACQ_MES && a.mes_ok) {
        if (feas) return fail(GP_ERR_ARG, "GP_ACQ_TIMES_FEAS: MES takes no probability of feasibility");
        if (a.mes_K < 1) return fail(GP_ERR_STATE, "GP_ACQ_MES without samples of the minimum's value (gp_mes_set)");
    } else if (base == GP_ACQ_POF && a.feas_ok) {
        if (!feas) return fail(GP_ERR_ARG, "GP_ACQ_POF is valid only together with GP_ACQ_TIMES_FEAS");
    } else if (base < GP_ACQ_EI || base > GP_ACQ_MPI) {
        return fail(GP_ERR_ARG, "unknown acquisition %d", a.type);
    }
    if (feas) {
        if (base == GP_ACQ_LCB) return fail(GP_ERR_ARG, "GP_ACQ_TIMES_FEAS: LCB takes no probability of feasibility");
        if (g->feas.K < 1 || g->feas.M != g->M)
            return fail(GP_ERR_ARG, "GP_ACQ_TIMES_FEAS without a probability of feasibility of the resident candidates (gp_feas_table)");
    }
    return check_per_cost(g, a.type, lp != nullptr);
}
// GP_ACQ_PER_COST: improvement per unit of cost is EI's and MPI's (LCB.py ignores the cost, LP.py:27 builds the penalised
// acquisition with unit cost), over a surface that is there
int check_per_cost(const gp_ctx *g, int type, bool lp) {
    if (!acq_per_cost(type)) return 0;
    GP_NO_LAPLACE(g, "GP_ACQ_PER_COST");
    if (acq_base(type) == GP_ACQ_LCB) return fail(GP_ERR_ARG, "GP_ACQ_PER_COST: LCB takes no cost");
    if (lp) return fail(GP_ERR_ARG, "GP_ACQ_PER_COST: the penalised acquisition takes no cost");
    if (g->cost.Nc < 1) return fail(GP_ERR_ARG, "GP_ACQ_PER_COST without a cost surface (gp_cost_set)");
    return 0;
}
int check_lp(const LpSpec &lp) {
    if (lp.transform != 0 && lp.transform != 1) return fail(GP_ERR_ARG, "transform must be 0 (none) or 1 (softplus)");
    if (lp.nb < 0 || lp.nb > GP_LP_MAX_NB) return fail(GP_ERR_ARG, "batch size out of range (0..%d)", GP_LP_MAX_NB);
    if (lp.nb > 0 && (!lp.Xb || !lp.r0 || !lp.s0)) return fail(GP_ERR_ARG, "null argument");
    return 0;
}
int check_sense(int sense) { return sense == 1 || sense == -1 ? 0 : fail(GP_ERR_ARG, "sense must be +1 or -1"); }
int check_k(int k) { return k >= 1 && k <= GP_TOPK_MAX ? 0 : fail(GP_ERR_ARG, "k out of range (1..%d)", GP_TOPK_MAX); }
int check_exclude(const int64_t *exclude, int nex, int64_t M) {   // rows already taken (run.py:1249-1252 masks them)
    if (nex < 0 || nex > GP_EXCLUDE_MAX) return fail(GP_ERR_ARG, "too many excluded rows (<= %d)", GP_EXCLUDE_MAX);
    if (nex > 0 && !exclude) return fail(GP_ERR_ARG, "null argument");
    for (int i = 0; i < nex; ++i)
        if (exclude[i] < 0 || exclude[i] >= M) return fail(GP_ERR_ARG, "excluded row out of range");
    return 0;
}

// ---- what every resident table shares (exact, sparse, ensemble, entropy search): scoring, selecting, handing over ------------
// arg-best: the two-level reduction into RED_RESULT
static void argbest_launch(gp_ctx *g, const double *v, long n, int sense) {
    launch_argbest(g->s, v, n, sense, g->dRedV + RED_RESULT.off, g->dRedI + RED_RESULT.off, g->dRedV + RED_PARTIAL.off,
                   g->dRedI + RED_PARTIAL.off);
}
// lowest index among the best of v[0, n), drained (idx may be null: the value alone)
int argbest_read(gp_ctx *g, const double *v, long n, int sense, int64_t *idx, double *val) {
    argbest_launch(g, v, n, sense);
    double hv = 0.0;
    long long hi = 0;
    HIPCHK(hipMemcpyAsync(&hv, g->dRedV + RED_RESULT.off, sizeof(double), hipMemcpyDeviceToHost, g->s));
    if (idx) HIPCHK(hipMemcpyAsync(&hi, g->dRedI + RED_RESULT.off, sizeof(long long), hipMemcpyDeviceToHost, g->s));
    GP_SYNC(g->s);
    *val = hv;
    if (idx) *idx = (int64_t)hi;
    return 0;
}

// The base acquisition of r's rows from their posterior -- value and x-gradient with grad --, then the log transform and the
// penaliser over the same buffers when lp is given (AcquisitionLP, GPyOpt/GPyOpt/acquisitions/LP.py:105-140).  No checks, no
// posterior: each model's preamble and its route to one come first.  Not drained.
int score_rows(gp_ctx *g, const AcqSpec &a, const LpSpec *lp, bool grad, const ScoreRows &r) {
    const int rule = acq_rule(a);
    if (rule == GP_ACQ_MES)   // (par and fmin are not read)
        launch_mes_acq(g->s, a.mes_y, a.mes_K, a.y_mean, a.y_std, r.mean, r.var, grad ? r.dm : nullptr, grad ? r.dv : nullptr, r.M, g->D,
                       r.acq, grad ? r.dacq : nullptr);
    else if (grad)
        launch_acq_grad(g->s, rule, a.par, a.fmin, a.y_mean, a.y_std, r.mean, r.var, r.dm, r.dv, r.M, g->D, r.acq, r.dacq);
    else if (rule != GP_ACQ_POF)
        launch_acq(g->s, rule, a.par, a.fmin, a.y_mean, a.y_std, r.mean, r.var, r.M, r.acq);
    // the probability of feasibility first, then the cost, then the penaliser's log transform (values of the resident table only:
    // check_acq)
    if (acq_times_feas(a)) feas_apply(g, rule == GP_ACQ_POF, r.acq);
    if (acq_per_cost(a.type)) return cost_divide(g, r.X, r.M, grad, r.acq, r.dacq);   // (never with lp: check_per_cost)
    if (!lp) return 0;
    int rc;
    LpBatch b;
    if ((rc = upload_lp_batch(g, *lp, &b))) return rc;   // (shared scratch: the upload resets the rows entries' batch cache)
    if (grad)
        launch_lp_grad(g->s, r.acq, r.dacq, r.X, r.M, g->D, b.X, lp->nb, b.r, b.s, lp->transform);
    else
        launch_lp(g->s, r.acq, r.X, r.M, g->D, b.X, lp->nb, b.r, b.s, lp->transform, r.acq);
    return 0;
}

// The winner among scores[0, M), the rows of exclude [nex] out of the running (run.py:1249-1252 masks the rows already taken)
int select_best(gp_ctx *g, double *scores, long M, int sense, const int64_t *exclude, int nex, int64_t *idx, double *val) {
    if (nex > 0) {
        long long *rows = g->dRedI + REDI_EXCLUDE.off;
        HIPCHK(hipMemcpyAsync(rows, exclude, sizeof(long long) * nex, hipMemcpyHostToDevice, g->s));
        launch_mask(g->s, scores, rows, nex, acq_empty(sense));
    }
    return argbest_read(g, scores, M, sense, idx, val);
}

// top-k of scores[0, M) (anchor_points_generator.py:61: argsort(scores)[:num_anchor]): k rounds of the deterministic arg-best
// reduction, each followed by masking the winner on the device: ties resolve to the lowest index in every round, i.e. the order
// of a stable sort by (score, index).
int select_topk(gp_ctx *g, double *scores, long M, int sense, int k, int64_t *idx, double *val) {
    int rc;
    if ((rc = g->dComm.reserve(COMM_CAP))) return rc;
    double *dv = g->dComm + COMM_TOPK_VAL.off;
    long long *di = (long long *)(g->dComm + COMM_TOPK_ROW.off);
    const int kk = (int)std::min<long>(k, M);
    for (int j = 0; j < kk; ++j) {
        argbest_launch(g, scores, M, sense);
        HIPCHK(hipMemcpyAsync(dv + j, g->dRedV + RED_RESULT.off, 8, hipMemcpyDeviceToDevice, g->s));
        HIPCHK(hipMemcpyAsync(di + j, g->dRedI + RED_RESULT.off, 8, hipMemcpyDeviceToDevice, g->s));
        launch_mask(g->s, scores, g->dRedI + RED_RESULT.off, 1, acq_empty(sense));
    }
    std::vector<long long> hi(kk);
    HIPCHK(hipMemcpyAsync(val, dv, sizeof(double) * kk, hipMemcpyDeviceToHost, g->s));
    HIPCHK(hipMemcpyAsync(hi.data(), di, sizeof(long long) * kk, hipMemcpyDeviceToHost, g->s));
    GP_SYNC(g->s);
    for (int j = 0; j < kk; ++j) idx[j] = (int64_t)hi[j];
    for (int j = kk; j < k; ++j) {  // fewer candidates than k: the tail is marked empty
        idx[j] = -1;
        val[j] = acq_empty(sense);
    }
    return 0;
}

// scores [M] (and their x-gradients [M, D]) to the caller, drained; a null destination is skipped
int scores_out(gp_ctx *g, const double *acq, const double *dacq, long M, int D, double *out, double *dout) {
    if (out) HIPCHK(hipMemcpyAsync(out, acq, sizeof(double) * M, hipMemcpyDeviceToHost, g->s));
    if (dout) HIPCHK(hipMemcpyAsync(dout, dacq, sizeof(double) * M * D, hipMemcpyDeviceToHost, g->s));
    GP_SYNC(g->s);
    return 0;
}

int train_values(gp_ctx *g) {
    GP_NO_LAPLACE(g, "gp_fmin");   // (y - d alpha: the targets of a Laplace fit are labels)
    // (a resident mean function: m(X_i) + r_i - d alpha_i = y_i - d alpha_i with the RAW targets; K alpha + m(X) directly)
    if (g->fmin_direct) {
        launch_train_mean(g->s, g->dX, g->N, g->kp, g->dAlpha, g->dMu);
        mean_add(g, g->dX, g->N, g->dMu);
    } else {
        launch_train_mean_identity(g->s, g->mean.on() ? g->dYraw : g->dY, g->dAlpha, g->noise + 1e-8 + g->jitter, g->N, g->dMu);
    }
    return 0;
}

extern "C" int gp_fmin(gp_t *g, double *fmin) {
    if (!g || !fmin) return fail(GP_ERR_ARG, "null argument");
    GP_FITTED(g);
    if (g->P != 1) return fail(GP_ERR_ARG, "gp_fmin needs P == 1");
    if (!g->fmin_valid) {
        int rc;
        if ((rc = train_values(g))) return rc;
        if ((rc = argbest_read(g, g->dMu, g->N, -1, nullptr, &g->fmin))) return rc;
        g->fmin_valid = true;
    }
    *fmin = g->fmin;
    return 0;
}

// The exact table's scores into dAcq (and dDacq with grad), not drained: the checks, the posterior with noise (GPModel.predict:
// with_noise=True, gpmodel.py:102) -- with grad the predictive gradients first, whose substitution route of a handful of rows
// leaves mean / variance behind --, then score_rows
int run_acq(gp_ctx *g, const AcqSpec &a, const LpSpec *lp, bool grad) {
    int rc;
    if (lp && (rc = check_lp(*lp))) return rc;
    if ((rc = check_acq(g, a, lp))) return rc;
    if ((rc = ensure_out(g))) return rc;
    if (grad && (rc = run_predict_grad(g))) return rc;
    if (!g->predicted || g->predicted_noise != 1)
        if ((rc = run_predict(g, 1))) return rc;
    return score_rows(g, a, lp, grad, ScoreRows{g->dXs, g->M, g->dMean, g->dVar, g->dDm, g->dDv, g->dAcq, g->dDacq});
}

extern "C" int gp_acq(gp_t *g, int type, double par, double fmin, double y_mean, double y_std, double *out) {
    if (!g || !out) return fail(GP_ERR_ARG, "null argument");
    GP_SCORING(g);
    return acq_values(g, exact_spec(g, AcqSpec{type, par, fmin, y_mean, y_std, true}), nullptr, out, nullptr);
}

// The winner among the resident candidates of the acquisition -- penalised when lp is given --, the rows of exclude [nex] out of
// the running (run.py:1249-1252 masks the rows already taken)
int acq_argbest(gp_ctx *g, const AcqSpec &a, const LpSpec *lp, int sense, const int64_t *exclude, int nex, int64_t *idx, double *val) {
    if (!g || !idx || !val) return fail(GP_ERR_ARG, "null argument");
    GP_SCORING(g);
    int rc;
    if ((rc = check_sense(sense))) return rc;
    if ((rc = check_exclude(exclude, nex, g->M))) return rc;
    if ((rc = run_acq(g, a, lp, false))) return rc;
    return select_best(g, g->dAcq, g->M, sense, exclude, nex, idx, val);
}

extern "C" int gp_acq_argbest(gp_t *g, int type, double par, double fmin, double y_mean, double y_std, int sense, int64_t *idx,
                   double *val) {
    return acq_argbest(g, exact_spec(g, AcqSpec{type, par, fmin, y_mean, y_std, true}), nullptr, sense, nullptr, 0, idx, val);
}

// ---- local penalisation (batch acquisition of run.py:1238-1257; GPyOpt/GPyOpt/acquisitions/LP.py) -----------
// the batch centres, radii and scales of the penaliser (<= 256 rows) in a small device buffer of their own
int upload_lp_batch(gp_ctx *g, const LpSpec &lp, LpBatch *b) {
    g->lp_cache_nb = -1;   // (api_rows.hip keeps the last batch it uploaded; this upload replaces it)
    int rc;
    if ((rc = g->dLp.reserve(LP_CAP))) return rc;
    *b = lp_slots(g);
    if (lp.nb > 0) {
        HIPCHK(hipMemcpyAsync(b->X, lp.Xb, sizeof(double) * lp.nb * g->D, hipMemcpyHostToDevice, g->s));
        HIPCHK(hipMemcpyAsync(b->r, lp.r0, sizeof(double) * lp.nb, hipMemcpyHostToDevice, g->s));
        HIPCHK(hipMemcpyAsync(b->s, lp.s0, sizeof(double) * lp.nb, hipMemcpyHostToDevice, g->s));
    }
    return 0;
}

extern "C" int gp_acq_lp(gp_t *g, int type, double par, double fmin, double y_mean, double y_std, int transform,
              const double *Xb, int nb, const double *r_x0, const double *s_x0, double *out) {
    if (!g || !out) return fail(GP_ERR_ARG, "null argument");
    GP_SCORING(g);
    const LpSpec lp{transform, Xb, nb, r_x0, s_x0};
    return acq_values(g, exact_spec(g, AcqSpec{type, par, fmin, y_mean, y_std, true}), &lp, out, nullptr);
}

extern "C" int gp_acq_lp_argbest(gp_t *g, int type, double par, double fmin, double y_mean, double y_std, int transform,
                      const double *Xb, int nb, const double *r_x0, const double *s_x0, int sense,
                      const int64_t *exclude, int nex, int64_t *idx, double *val) {
    const LpSpec lp{transform, Xb, nb, r_x0, s_x0};
    return acq_argbest(g, exact_spec(g, AcqSpec{type, par, fmin, y_mean, y_std, true}), &lp, sense, exclude, nex, idx, val);
}

// full_cov = True branch of PosteriorExact._raw_predict (posterior.py:280-284)
extern "C" int gp_predict_full_cov(gp_t *g, int include_noise, double *mean, double *cov) {
    if (!g || !cov) return fail(GP_ERR_ARG, "null argument");
    GP_SCORING(g);
    const long M = g->M, Npad = g->Npad, Mpad = round_up(M, GP_TILE);
    if (Mpad > g->mc_max) return fail(GP_ERR_ARG, "full covariance needs M <= mc_max (%ld)", g->mc_max);
    int rc;
    if ((rc = ensure_out(g))) return rc;
    if ((rc = run_predict(g, include_noise, true))) return rc;  // leaves S = K(Xs,X) L^-T in dT2 (single chunk, zero padding rows: tile path)
    if ((rc = g->dCov.reserve(Mpad * Mpad))) return rc;
    const int mt = (int)(Mpad / GP_TILE);
    launch_kbuild(g->s, g->dCov, Mpad, g->dXs, M, Mpad, g->kp, 0.0, 1);  // K(Xs, Xs)
    gemm(g, g->s, 1, g->dCov, Mpad, g->dT2, Npad, g->dT2, Npad, 1, (int)Npad, TileSet{0, mt, 0, mt, 0});
    if (include_noise) launch_add_diag(g->s, g->dCov, Mpad, M, g->noise);  // gaussian.py:104-105
    if (mean) HIPCHK(hipMemcpyAsync(mean, g->dMean, sizeof(double) * M * g->P, hipMemcpyDeviceToHost, g->s));
    GP_SYNC(g->s);
    HIPCHK(hipMemcpy2D(cov, sizeof(double) * M, g->dCov, sizeof(double) * Mpad, sizeof(double) * M, M,
                       hipMemcpyDeviceToHost));
    return 0;
}

// ---- top-k of the acquisition scores --------------------------------------------------------------------------------
int acq_topk(gp_ctx *g, const AcqSpec &a, int sense, int k, int64_t *idx, double *val) {
    if (!g || !idx || !val) return fail(GP_ERR_ARG, "null argument");
    GP_SCORING(g);
    int rc;
    if ((rc = check_sense(sense))) return rc;
    if ((rc = check_k(k))) return rc;
    if ((rc = run_acq(g, a, nullptr, false))) return rc;
    return select_topk(g, g->dAcq, g->M, sense, k, idx, val);
}

extern "C" int gp_acq_topk(gp_t *g, int type, double par, double fmin, double y_mean, double y_std, int sense, int k,
                int64_t *idx, double *val) {
    return acq_topk(g, exact_spec(g, AcqSpec{type, par, fmin, y_mean, y_std, true}), sense, k, idx, val);
}

// ---- posterior samples of the latent function (GP.posterior_samples_f, gp.py:581-609) ------------------------
// dev[s, :] = C z_s with C C^T = cov(Xs) (+ noise I) the full posterior covariance (posterior.py:280-284) of the resident
// candidates and z_s the caller's standard normals: the M x M Cholesky runs on the device with the same tile kernels as
// the fit, under GPy's jitter ladder (jitchol, linalg.py:56-81).  mean[M,P] is returned beside the deviations; a sample
// of output d is mean[:, d] + dev[s, :].  (The reference draws through numpy's multivariate_normal, whose SVD factor
// differs from C by an orthogonal matrix: same distribution, different draws for the same generator state.)
extern "C" int gp_posterior_samples(gp_t *g, int include_noise, const double *Z, int S, int maxtries, double *mean, double *dev,
                         double *jitter_used) {
    if (!g || !Z || !dev) return fail(GP_ERR_ARG, "null argument");
    GP_SCORING(g);
    if (S < 1) return fail(GP_ERR_ARG, "S < 1");
    const long M = g->M, Npad = g->Npad, Mpad = round_up(M, GP_TILE), Spad = round_up(S, GP_TILE);
    if (Mpad > g->mc_max) return fail(GP_ERR_ARG, "posterior samples need M <= mc_max (%ld)", g->mc_max);
    int rc;
    if ((rc = ensure_out(g))) return rc;
    if ((rc = run_predict(g, include_noise, true))) return rc;  // S_c = K(Xs,X) L^-T in dT2 (single chunk, zero padding rows: tile path), mean in dMean
    // dCov: [cov Mpad x Mpad][Z^T Spad x Mpad][dev Spad x Mpad]; the inverted diagonal tiles go to dT (free now)
    if ((rc = g->dCov.reserve(Mpad * Mpad + 2 * Spad * Mpad))) return rc;
    double *C = g->dCov, *Zd = g->dCov + Mpad * Mpad, *Dv = Zd + Spad * Mpad;
    double *invL = g->dT;
    const int mt = (int)(Mpad / GP_TILE), st = (int)(Spad / GP_TILE);
    HIPCHK(hipMemsetAsync(Zd, 0, sizeof(double) * Spad * Mpad, g->s));
    // (the diagonal-tile kernel writes the lower block triangle of an inverted tile only; dT held candidate rows before)
    HIPCHK(hipMemsetAsync(invL, 0, sizeof(double) * Mpad * GP_TILE, g->s));
    HIPCHK(hipMemcpy2DAsync(Zd, sizeof(double) * Mpad, Z, sizeof(double) * M, sizeof(double) * M, S,
                            hipMemcpyHostToDevice, g->s));
    // jitchol scales its ladder by the mean of the diagonal of the matrix it factors (linalg.py:62-66: diagA.mean() * 1e-6):
    // here the POSTERIOR covariance, whose diagonal near training points is orders of magnitude below the prior variance
    double diag_stat[2] = {0.0, 0.0};   // trace and smallest entry of the diagonal of the matrix to factor
    double jitter = 0.0;
    int tries = 0;
    for (int info = 0, bad = 0;;) {
        launch_kbuild(g->s, C, Mpad, g->dXs, M, Mpad, g->kp, 0.0, 1);  // K(Xs, Xs), identity on the padding rows
        gemm(g, g->s, 1, C, Mpad, g->dT2, Npad, g->dT2, Npad, 1, (int)Npad, TileSet{0, mt, 0, mt, 0});
        if (include_noise) launch_add_diag(g->s, C, Mpad, M, g->noise);
        if (tries == 0) {
            launch_trace(g->s, C, Mpad, M, g->dScal + SCAL_TRACE.off);
            HIPCHK(hipMemcpyAsync(diag_stat, g->dScal + SCAL_TRACE.off, sizeof diag_stat, hipMemcpyDeviceToHost, g->s));
        }
        if (jitter != 0.0) launch_add_diag(g->s, C, Mpad, M, jitter);
        HIPCHK(hipMemsetAsync(g->dInfo, 0, sizeof(int) * 4, g->s));
        Members cov;   // one member: the posterior covariance, no RHS rows
        cov.A = C;
        cov.lda = Mpad;
        cov.invL = invL;
        cov.info = g->dInfo;
        factor_buf(g, cov, mt, mt);
        if ((rc = factor_status(g, g->emulate_fp64, &info, &bad))) return rc;
        if (bad) return fail(GP_ERR_STATE, "emulate_fp64: an entry of L left the fixed-point range");
        if (info == 0) break;
        // np.any(diagA <= 0.) raises before any jitter is tried (linalg.py:61-62): ANY entry, not the mean -- a posterior
        // variance that came out slightly negative at a training point is such an entry
        if (diag_stat[1] <= 0.0) return fail(GP_ERR_NOT_PD_DIAG, "not pd: non-positive diagonal elements");
        // jitchol: mean(diag) * 1e-6 * 10^k (linalg.py:62-75)
        const int rcl = ladder_step(diag_stat[0] / (double)M, maxtries, info, &jitter, &tries);
        if (rcl == GP_ERR_NOT_PD_DIAG) return fail(rcl, "not pd: non-positive diagonal elements");
        if (rcl) {
            g_err = "not positive definite, even with jitter.";
            return rcl;
        }
    }
    launch_zero_upper_diag(g->s, C, Mpad, mt);
    // dev[s, m] = sum_{k <= m} z[s, k] C[m, k]: B = the factor's rows, contraction ends at the diagonal tile
    GemmOpt o;
    o.k_end_tri = 1;
    gemm(g, g->s, 0, Dv, Mpad, Zd, Mpad, C, Mpad, 1, (int)Mpad, TileSet{0, st, 0, mt, 0}, o);
    if (mean) HIPCHK(hipMemcpyAsync(mean, g->dMean, sizeof(double) * M * g->P, hipMemcpyDeviceToHost, g->s));
    HIPCHK(hipMemcpy2DAsync(dev, sizeof(double) * M, Dv, sizeof(double) * Mpad, sizeof(double) * M, S,
                            hipMemcpyDeviceToHost, g->s));
    GP_SYNC(g->s);
    if (jitter_used) *jitter_used = jitter;
    g->predicted = false;  // dT was used as workspace
    return 0;
}
