// A handful of locations per call, answered in one entry point: what scipy's L-BFGS-B asks of the acquisition between two fits
// (GPyOpt/GPyOpt/optimization/optimizer.py:36-61 -> acquisitions/base.py:33-50, LP.py:105-140 -> models/gpmodel.py:95-142 ->
// GPy/GPy/core/gp.py:297-354,407-454).  The fused path (onerow.hip) takes the locations BY VALUE and returns through a pinned
// result block; everything it cannot take goes through gp_set_candidates + the batched entry points, same results.
#include "api_internal.h"

// fused path: up to 8 locations of a single-output model whose coordinates fit the kernel arguments -- of each pass, that is: four
// locations at a time (ROWS_MAX_M), or all of 5 .. 8 in one wide pass when M * D fits as a whole (rows_pass_width)
static bool rows_fused_ok(const gp_ctx *g, int64_t M) {
    return g->small_m > 0 && M >= 1 && M <= g->small_m && g->P == 1 && (long)std::min<int64_t>(M, ROWS_MAX_M) * g->D <= ROWS_MAX_XS;
}

// Locations per pass of an M-location call: M itself while one pass can take them -- up to ROWS_MAX_M always, up to ROWS_WIDE_M
// where the wide instances are on (option "rows_wide") and M * D coordinates fit the kernel arguments -- else ROWS_MAX_M.
static int rows_pass_width(const gp_ctx *g, int M) {
    if (M <= ROWS_MAX_M) return M;
    return g->rows_wide && M <= ROWS_WIDE_M && (long)M * g->D <= ROWS_MAX_XS ? M : ROWS_MAX_M;
}

// When to build the inverse factor (N^3 / 3 flops once per fit: 0.7 ms at N = 4096, 4.4 ms at N = 8192, 28 ms at N = 16384).  A gradient
// call through the substitution route (~90 short launches against L, no precomputation) costs 1.84 ms at N = 16384 against 0.44 fused
// (0.55 against 0.16 at N = 8192), so the factor pays for itself after build / (substitution - fused) = ~20 calls at N = 16384, ~11 at
// N = 8192: about nt / 6 at either size.  Not knowing how many calls will follow a fit, the rule is the ski-rental one -- rent until
// the rent paid equals the price: the first nt / 6 calls after a fit take the substitution route, the next one builds the factor
// (never worse than twice the best choice in hindsight).  Small matrices (N <= 4096) build at the first call; a factor that exists is
// always used.
static bool rows_use_factor(gp_ctx *g) {
    if (g->li_valid || g->N <= 4096 || g->rows_build == 1) return true;
    if (g->rows_build == 0) return false;
    return ++g->rows_calls_since_fit > g->Npad / GP_TILE / 6;
}

int rows_scratch(gp_ctx *g, RowsWork *w) {
    const long Npad = g->Npad;
    const int nt = (int)(Npad / GP_TILE);
    const long nch = nt > 0 ? (nt - 1) / 8 + 1 : 1;
    const long nrb = (long)nt * (GP_TILE / rows_block_height(nt));   // row blocks of the backward pass
    // sized for a wide pass; a pass lays its partials out for its own MV (rows_layout) from the front of each array
    const long n_w = nch * ROWS_WIDE_M * Npad, n_b = nrb * ROWS_WIDE_M * Npad, n_m = nch * ROWS_WIDE_M, n_v = nrb * ROWS_WIDE_M;
    const long n_g = (long)rows_gpart_elems(g->N);
    int rc;
    if ((rc = g->dRows.reserve(n_w + n_b + n_m + n_v + n_g))) return rc;
    w->wpart = g->dRows;
    w->bpart = w->wpart + n_w;
    w->meanpart = w->bpart + n_b;
    w->vpart = w->meanpart + n_m;
    w->gpart = w->vpart + n_v;
    return g->pass.ready(g->s);
}

// the penaliser's batch on the device; re-uploaded only when it changed (an L-BFGS run keeps one batch for hundreds of calls)
int rows_lp_batch(gp_ctx *g, const LpSpec &lp, LpBatch *b) {
    const int nb = lp.nb;
    const size_t nx = (size_t)nb * g->D;
    bool same = g->lp_cache_nb == nb && g->lp_cache.size() == nx + 2 * (size_t)nb && g->dLp;
    if (same && nb > 0)
        same = !memcmp(g->lp_cache.data(), lp.Xb, sizeof(double) * nx) && !memcmp(g->lp_cache.data() + nx, lp.r0, sizeof(double) * nb) &&
               !memcmp(g->lp_cache.data() + nx + nb, lp.s0, sizeof(double) * nb);
    if (same) {
        *b = lp_slots(g);
        return 0;
    }
    int rc;
    if ((rc = upload_lp_batch(g, lp, b))) return rc;
    g->lp_cache.resize(nx + 2 * (size_t)nb);
    if (nb > 0) {
        memcpy(g->lp_cache.data(), lp.Xb, sizeof(double) * nx);
        memcpy(g->lp_cache.data() + nx, lp.r0, sizeof(double) * nb);
        memcpy(g->lp_cache.data() + nx + nb, lp.s0, sizeof(double) * nb);
    }
    g->lp_cache_nb = nb;
    return 0;
}

RowsAcq rows_acq(const AcqSpec &a, const LpSpec *lp, const LpBatch &b) {   // (RowsAcq: on, the base acquisition, lp, the penaliser)
    if (!lp) return RowsAcq{1, acq_base(a.type), a.par, a.fmin, a.y_mean, a.y_std, 0, 0, 0, nullptr, nullptr, nullptr, a.mes_y, a.mes_K};
    return RowsAcq{1, acq_base(a.type), a.par, a.fmin, a.y_mean, a.y_std, 1, lp->transform, lp->nb, b.X, b.r, b.s, a.mes_y, a.mes_K};
}

// The exact model's passes through rows_passes (api_internal.h): rows_pass_width locations per pass.  launch(rx, w, r) puts a pass
// on the stream and returns how many workgroups arrive at its counter; unpack(m0, mc, MV, o) takes the results of locations
// [m0, m0 + mc) out of the pinned block o, laid out for MV locations (gphip_internal.h).  With a phase name a profiled context
// times each pass: `cost` reads of the inverse factor's triangle, and as many N^2 products per location.
template <class Launch, class Unpack>
static int rows_exact_passes(gp_ctx *g, const double *Xs, int M, const char *phase, double cost, Launch launch, Unpack unpack) {
    int rc;
    RowsWork w;
    if ((rc = rows_scratch(g, &w))) return rc;
    const bool timed = phase && g->profiling;
    if (timed) g->nphases = 0;
    rc = rows_passes(
        g, g->pass, Xs, M, rows_pass_width(g, M),
        [&](const RowsX &rx, const PassReport &r, unsigned *arrivals) {
            const int ph = timed ? phase_begin(g, phase, cost * (double)g->N * g->N * rx.M, cost * 8.0 * (double)g->N * g->N / 2) : -1;
            arrivals[0] = launch(rx, w, r);
            if (timed) phase_end(g, ph);
            return 0;
        },
        [&](int m0, int mc, const double *o) {
            ++(mc > ROWS_MAX_M ? g->rows_wide_passes : g->rows_narrow_passes);
            unpack(m0, mc, rows_layout(mc), o);
        });
    if (!rc) ++g->rows_fused_calls;
    return rc;
}

// The fused path over the inverse factor.  want_grad selects forward + backward + finish; otherwise forward + finish.
// Results: mean / var / acq [M], dmdx / dvdx / dacq [M, D] (any may be null).
static int rows_fused(gp_ctx *g, const double *Xs, int M, int include_noise, int want_grad, const RowsAcq &aq, double *mean,
                      double *var, double *acq, double *dmdx, double *dvdx, double *dacq, bool per_cost = false) {
    int rc;
    if ((rc = ensure_linv(g))) return rc;
    return rows_exact_passes(
        g, Xs, M, want_grad ? "rows_fused_grad" : "rows_fused", want_grad ? 2.0 : 1.0,
        [&](const RowsX &rx, const RowsWork &w, const PassReport &r) {
            launch_rows(g->s, g->dLi, g->Npad, rx, g->kp, g->dX, g->N, g->dAlpha, want_grad, g->kp.variance,
                        include_noise ? g->noise : 0.0, aq, w, r, g->rows_nt < 0 ? (g->Npad > 8192 ? 1 : 0) : g->rows_nt, rows_mean(g));
            if (per_cost) cost_divide_block(g, rx, want_grad != 0, r.out, rows_layout(rx.M));   // behind the pass, before the drain
            return rows_finish_grid(g->N);
        },
        [&](int m0, int mc, int MV, const double *o) { rows_unpack(o, MV, m0, mc, g->D, mean, var, acq, dmdx, dvdx, dacq); });
}

// What api_feas.hip sequences: several handles' passes of one device behind each other on the shared stream, one drain at the end
bool rows_take_fused(gp_ctx *g, int64_t M) { return rows_fused_ok(g, M) && rows_use_factor(g); }
int rows_prepare(gp_ctx *g) {
    int rc;
    if ((rc = ensure_linv(g))) return rc;
    RowsWork w;
    return rows_scratch(g, &w);
}
void rows_enqueue(gp_ctx *g, const RowsX &rx, int include_noise, int want_grad, const RowsAcq &aq, PassReport *r, unsigned *arrivals) {
    RowsWork w;
    (void)rows_scratch(g, &w);   // (reserved by rows_prepare: the pointers alone)
    *r = g->pass.next();
    launch_rows(g->s, g->dLi, g->Npad, rx, g->kp, g->dX, g->N, g->dAlpha, want_grad, g->kp.variance, include_noise ? g->noise : 0.0,
                aq, w, *r, g->rows_nt < 0 ? (g->Npad > 8192 ? 1 : 0) : g->rows_nt, rows_mean(g));
    *arrivals = rows_finish_grid(g->N);
    ++(rx.M > ROWS_MAX_M ? g->rows_wide_passes : g->rows_narrow_passes);
}

// The posterior of a handful of locations: gp_set_candidates + gp_predict (+ gp_predict_grad when dmdx / dvdx are given) as ONE
// call (PosteriorExact._raw_predict, posterior.py:273-302; GP.predictive_gradients, gp.py:407-454).
extern "C" int gp_predict_rows(gp_t *g, const double *Xs, int64_t M, int include_noise, double *mean, double *var, double *dmdx,
                               double *dvdx) {
    if (!g || !Xs) return fail(GP_ERR_ARG, "null argument");
    GP_FITTED(g);
    if (M < 1) return fail(GP_ERR_ARG, "M < 1");
    if (dvdx && !dmdx) return fail(GP_ERR_ARG, "dvdx needs dmdx");
    if (dmdx && !dvdx && (mean || var)) return fail(GP_ERR_ARG, "the mean's gradient alone (dvdx NULL) comes without mean / var");
    int rc;
    if (dmdx && !dvdx) {
        // d mean / dx alone: one pass over the training points, no inverse factor, no substitutions (estimate_L's inner call)
        if (rows_fused_ok(g, M)) {
            const int D = g->D;
            return rows_exact_passes(
                g, Xs, (int)M, nullptr, 0.0,
                [&](const RowsX &rx, const RowsWork &w, const PassReport &r) {
                    launch_rows_mean_grad(g->s, rx, g->kp, g->dX, g->N, g->dAlpha, w, r, rows_mean(g));
                    return rows_mean_grad_grid(g->N);
                },
                [&](int m0, int mc, int MV, const double *o) { memcpy(dmdx + (long)m0 * D, o + 3 * MV, sizeof(double) * mc * D); });
        }
        ++g->rows_fallback_calls;
        if ((rc = gp_set_candidates(g, Xs, M))) return rc;
        return gp_predict_grad(g, dmdx, nullptr);
    }
    const int want_grad = dmdx != nullptr;
    if (rows_fused_ok(g, M) && rows_use_factor(g)) {
        RowsAcq aq{};
        return rows_fused(g, Xs, (int)M, include_noise, want_grad, aq, mean, var, nullptr, dmdx, dvdx, nullptr);
    }
    ++g->rows_fallback_calls;
    if ((rc = gp_set_candidates(g, Xs, M))) return rc;
    if (mean || var)
        if ((rc = gp_predict(g, include_noise, mean, var))) return rc;
    if (want_grad)
        if ((rc = gp_predict_grad(g, dmdx, dvdx))) return rc;
    return 0;
}

// The (negated) acquisition at a handful of locations and, when dout is given, its x-gradient: gp_set_candidates + gp_acq /
// gp_acq_grad (lp = 0; acquisitions/base.py:33-50) or gp_acq_lp / gp_acq_lp_grad (lp = 1; LP.py:105-140) as ONE call.
extern "C" int gp_acq_rows(gp_t *g, const double *Xs, int64_t M, int type, double par, double fmin, double y_mean, double y_std,
                           int lp, int transform, const double *Xb, int nb, const double *r_x0, const double *s_x0, double *out,
                           double *dout) {
    if (!g || !Xs || !out) return fail(GP_ERR_ARG, "null argument");
    GP_FITTED(g);
    if (M < 1) return fail(GP_ERR_ARG, "M < 1");
    const AcqSpec a = exact_spec(g, AcqSpec{type, par, fmin, y_mean, y_std});
    const LpSpec batch{transform, Xb, nb, r_x0, s_x0}, *pen = lp ? &batch : nullptr;
    int rc;
    if ((rc = check_acq(g, a, pen))) return rc;
    if (pen && (rc = check_lp(*pen))) return rc;
    if (rows_fused_ok(g, M) && rows_use_factor(g)) {
        LpBatch b;
        if (pen && (rc = rows_lp_batch(g, *pen, &b))) return rc;
        return rows_fused(g, Xs, (int)M, 1, dout != nullptr, rows_acq(a, pen, b), nullptr, nullptr, out, nullptr, nullptr,
                          dout, acq_per_cost(type));   // with_noise=True, gpmodel.py:102
    }
    ++g->rows_fallback_calls;
    if ((rc = gp_set_candidates(g, Xs, M))) return rc;
    return acq_values(g, a, pen, out, dout);
}

// gp_es_acq for a handful of locations given by value (ES has no analytic gradient: L-BFGS-B runs on differences, D + 1
// one-location calls per step).  Fused: the forward pass over the inverse factor as for every rows call, then ONE kernel that
// forms C = k(x, Xr) - V_R w, the variance and the score and reports through the pass's owner (csrc/es.hip).
extern "C" int gp_es_acq_rows(gp_t *g, const double *Xs, int64_t M, double y_std, double *out) {
    if (!g || !Xs || !out) return fail(GP_ERR_ARG, "null argument");
    GP_FITTED(g);
    GP_NO_MEAN(g, "gp_es_acq_rows");
    if (M < 1) return fail(GP_ERR_ARG, "M < 1");
    int rc;
    if ((rc = es_ready(g, y_std))) return rc;
    if (rows_fused_ok(g, M) && rows_use_factor(g)) {
        if ((rc = ensure_linv(g))) return rc;
        EsState &es = g->es;
        if ((rc = es.dRowsPart.reserve((long)es_rows_part_elems(g->Npad)))) return rc;
        const EsBelief b = es_belief(g);
        return rows_exact_passes(
            g, Xs, (int)M, "rows_es", 1.0,
            [&](const RowsX &rx, const RowsWork &w, const PassReport &r) {
                launch_rows_forward(g->s, g->dLi, g->Npad, rx, g->kp, g->dX, g->N, g->dAlpha, w,
                                    g->rows_nt < 0 ? (g->Npad > 8192 ? 1 : 0) : g->rows_nt);
                launch_es_rows(g->s, rx, g->kp, es.dXr, es.R, es.dVR, g->Npad, w.wpart, es.dRowsPart, g->kp.variance, y_std, b.Qt, b.Gt,
                               b.logP, b.u, b.W, es.S, r);
                return es_rows_grid(g->Npad);
            },
            [&](int m0, int mc, int MV, const double *o) { rows_unpack(o, MV, m0, mc, g->D, nullptr, nullptr, out, nullptr, nullptr, nullptr); });
    }
    ++g->rows_fallback_calls;
    if ((rc = gp_set_candidates(g, Xs, M))) return rc;
    return gp_es_acq(g, y_std, out);
}

// The knowledge gradient at a handful of locations given by value, negated as gp_acq_rows returns its scores, and with dout its
// closed-form gradient (kernels: csrc/kg.hip).  Fused: the forward pass over the inverse factor, the shares of C = k(x, X_A) - V_A w
// and a scoring launch of one workgroup per location that leaves the adjoint coefficients; for a gradient the coefficients are mixed into the backward
// pass's right-hand sides, so that the UNCHANGED backward pass reads the inverse factor once more, and a closing pass over the
// training points ends the call.  Beyond the fused path: the two table calls, values only.
extern "C" int gp_kg_rows(gp_t *g, const double *Xs, int64_t M, double y_std, double *out, double *dout) {
    if (!g || !Xs || !out) return fail(GP_ERR_ARG, "null argument");
    GP_FITTED(g);
    GP_NO_MEAN(g, "gp_kg_rows");
    if (M < 1) return fail(GP_ERR_ARG, "M < 1");
    int rc;
    if ((rc = kg_ready(g, y_std))) return rc;
    for (int64_t i = 0; i < M * g->D; ++i)
        if (!std::isfinite(Xs[i])) return fail(GP_ERR_ARG, "gp_kg_rows: a location is not finite");
    const bool fused = rows_fused_ok(g, M);
    if (dout && !fused) return fail(GP_ERR_ARG, "gp_kg_rows: the gradient needs a shape the fused rows path takes (M <= %ld)", g->small_m);
    // the build policy's counter moves with every call the fused path could take, as in gp_acq_rows; a gradient call takes the
    // factor whatever the policy says (built at the first one)
    const bool factor = fused && rows_use_factor(g);
    if (fused && (dout || factor)) {
        if ((rc = ensure_linv(g))) return rc;
        KgState &kg = g->kg;
        if ((rc = kg.dRowsPart.reserve((long)kg_rows_part_elems(g->Npad)))) return rc;
        if ((rc = kg.dState.reserve((long)ROWS_WIDE_M * KG_STATE_STRIDE))) return rc;
        const int want_grad = dout != nullptr;
        const int nt_loads = g->rows_nt < 0 ? (g->Npad > 8192 ? 1 : 0) : g->rows_nt;
        return rows_exact_passes(
            g, Xs, (int)M, want_grad ? "rows_kg_grad" : "rows_kg", want_grad ? 2.0 : 1.0,
            [&](const RowsX &rx, const RowsWork &w, const PassReport &r) {
                launch_rows_forward(g->s, g->dLi, g->Npad, rx, g->kp, g->dX, g->N, g->dAlpha, w, nt_loads);
                launch_kg_rows(g->s, rx, g->kp, kg.dXa, kg.A, kg.dVA, kg.dMuA, g->Npad, w, kg.dRowsPart, g->kp.variance, g->noise, y_std,
                               want_grad, kg.dState, r);
                unsigned arrivals = (unsigned)rx.M;   // the scoring kernel: one workgroup per location
                if (want_grad) {
                    launch_kg_mix(g->s, rx.M, g->N, g->Npad, w, kg.dVA, kg.A, kg.dState);
                    launch_rows_backward(g->s, g->dLi, g->Npad, rx.M, w, nt_loads);
                    launch_kg_close(g->s, rx, g->kp, g->dX, g->N, g->Npad, g->dAlpha, w, kg.dXa, kg.A, kg.dState, r, r.base + arrivals);
                    arrivals += rows_finish_grid(g->N);
                }
                return arrivals;
            },
            [&](int m0, int mc, int MV, const double *o) { rows_unpack(o, MV, m0, mc, g->D, nullptr, nullptr, out, nullptr, nullptr, dout); });
    }
    ++g->rows_fallback_calls;
    if ((rc = gp_set_candidates(g, Xs, M))) return rc;
    if ((rc = gp_kg_acq(g, y_std, out))) return rc;
    for (int64_t i = 0; i < M; ++i) out[i] = -out[i];
    return 0;
}

// Noisy expected improvement at a handful of locations given by value, on the TWIN, negated as gp_acq_rows returns its scores, and
// with dout its closed-form gradient (kernels: csrc/nei.hip).  Fused: the forward pass over the twin's inverse factor, the shares
// of k . a_s and |w|^2, and a scoring launch of one workgroup per location that leaves p and c; for a gradient the adjoint
// w' = cw w + sum_s cv_s U_s (U = L0^-1 F, so that L0^-T w' = cw beta_x - y_std A0 p) is mixed into the right-hand sides of the
// UNCHANGED backward pass by the knowledge gradient's mix kernel, and its closing pass, without cross terms, ends the call: the
// inverse factor is read twice whatever S.  Beyond the fused path: the table route, values only.
extern "C" int gp_nei_rows(gp_t *g, const double *Xs, int64_t M, double par, double y_mean, double y_std, double *out, double *dout) {
    if (!g || !Xs || !out) return fail(GP_ERR_ARG, "null argument");
    GP_FITTED(g);
    if (M < 1) return fail(GP_ERR_ARG, "M < 1");
    int rc;
    if ((rc = nei_ready(g, y_mean, y_std, "gp_nei_rows"))) return rc;
    if (!std::isfinite(par)) return fail(GP_ERR_ARG, "gp_nei_rows: par must be finite");
    for (int64_t i = 0; i < M * g->D; ++i)
        if (!std::isfinite(Xs[i])) return fail(GP_ERR_ARG, "gp_nei_rows: a location is not finite");
    const bool fused = rows_fused_ok(g, M);
    if (dout && !fused) return fail(GP_ERR_ARG, "gp_nei_rows: the gradient needs a shape the fused rows path takes (M <= %ld)", g->small_m);
    // the build policy's counter moves with every call the fused path could take, as in gp_acq_rows; a gradient call takes the
    // factor whatever the policy says (built at the first one)
    const bool factor = fused && rows_use_factor(g);
    if (fused && (dout || factor)) {
        if ((rc = ensure_linv(g))) return rc;
        NeiState &ne = g->nei;
        if ((rc = ne.dRowsPart.reserve((long)nei_rows_part_elems(g->Npad)))) return rc;
        if ((rc = ne.dState.reserve((long)ROWS_WIDE_M * KG_STATE_STRIDE))) return rc;
        const int want_grad = dout != nullptr;
        const int nt_loads = g->rows_nt < 0 ? (g->Npad > 8192 ? 1 : 0) : g->rows_nt;
        return rows_exact_passes(
            g, Xs, (int)M, want_grad ? "rows_nei_grad" : "rows_nei", want_grad ? 2.0 : 1.0,
            [&](const RowsX &rx, const RowsWork &w, const PassReport &r) {
                // every kernel of the pass is counted where it is launched, and so is every one that reads g->dLi (gp_nei_stats)
                int launches = 0, reads = 0;
                launch_rows_forward(g->s, g->dLi, g->Npad, rx, g->kp, g->dX, g->N, g->dAlpha, w, nt_loads);
                ++launches, ++reads;
                launches += launch_nei_rows(g->s, rx, g->kp, g->dX, g->N, g->Npad, ne.dA0, ne.S, ne.dFstar, w, ne.dRowsPart, g->kp.variance,
                                            g->noise, par, y_mean, y_std, want_grad, ne.dState, r);
                unsigned arrivals = (unsigned)rx.M;   // the scoring kernel: one workgroup per location
                if (want_grad) {
                    launch_kg_mix(g->s, rx.M, g->N, g->Npad, w, ne.dU, ne.S, ne.dState);
                    ++launches;
                    launch_rows_backward(g->s, g->dLi, g->Npad, rx.M, w, nt_loads);
                    ++launches, ++reads;
                    launch_kg_close(g->s, rx, g->kp, g->dX, g->N, g->Npad, g->dAlpha, w, nullptr, 0, ne.dState, r, r.base + arrivals);
                    ++launches;
                    arrivals += rows_finish_grid(g->N);
                }
                ne.pass_launches = launches;
                ne.pass_reads = reads;
                return arrivals;
            },
            [&](int m0, int mc, int MV, const double *o) { rows_unpack(o, MV, m0, mc, g->D, nullptr, nullptr, out, nullptr, nullptr, dout); });
    }
    ++g->rows_fallback_calls;
    g->nei.pass_launches = g->nei.pass_reads = 0;
    if ((rc = gp_set_candidates(g, Xs, M))) return rc;
    if ((rc = gp_nei_table(g, par, y_mean, y_std, out))) return rc;
    for (int64_t i = 0; i < M; ++i) out[i] = -out[i];
    return 0;
}

// how many *_rows calls took the fused path / the batched entry points since the context was created (route checks in tests)
extern "C" int gp_rows_stats(gp_t *g, int64_t *fused, int64_t *fallback) {
    if (!g) return fail(GP_ERR_ARG, "null gp");
    if (fused) *fused = g->rows_fused_calls;
    if (fallback) *fallback = g->rows_fallback_calls;
    return 0;
}

// how many passes of at most ROWS_MAX_M locations / wide passes the fused path has made since the context was created (route check)
extern "C" int gp_rows_pass_stats(gp_t *g, int64_t *narrow, int64_t *wide) {
    if (!g) return fail(GP_ERR_ARG, "null gp");
    if (narrow) *narrow = g->rows_narrow_passes;
    if (wide) *wide = g->rows_wide_passes;
    return 0;
}
