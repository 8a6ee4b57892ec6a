// Black-box constraints: constraints known only through evaluations, each modelled by an exact GP of its own, and EI / MPI weighted
// by the probability of feasibility  F(x) = prod_k Phi((b_k - m_k(x)) / s_k(x))  (Gardner et al. 2014; Gelbart et al. 2014).
// Unlike the cost (api_cost.hip) F needs each constraint GP's VARIANCE, so every constraint stays a live handle with its factor;
// the scored handle caches only log F over its resident table.  Contexts of one device share one stream set (DevStreams): the
// handles of a call are sequenced on that stream and drained once.
#include "api_internal.h"

namespace {
struct FeasIn {
    int K;
    gp_ctx *c[GP_FEAS_MAX];
    const double *bound, *c_mean, *c_std;
};

// the constraint handles of a call against the device, stream and width they have to share (gp: the scored handle, or null)
int check_cons(const gp_ctx *gp, gp_t *const *cons, int K, const double *bound, const double *c_mean, const double *c_std, FeasIn *in) {
    if (K < 1 || K > GP_FEAS_MAX) return fail(GP_ERR_ARG, "K out of range (1..%d)", GP_FEAS_MAX);
    if (!cons || !bound || !c_mean || !c_std) return fail(GP_ERR_ARG, "null argument");
    for (int k = 0; k < K; ++k) {
        gp_ctx *c = cons[k];
        if (!c) return fail(GP_ERR_ARG, "null constraint handle (%d)", k);
        GP_DEAD_CHECK(c);
        const gp_ctx *ref = gp ? gp : cons[0];
        if (c == gp) return fail(GP_ERR_ARG, "constraint %d is the scored handle itself", k);
        for (int j = 0; j < k; ++j)
            if (cons[j] == c) return fail(GP_ERR_ARG, "constraint handle %d is listed twice", k);
        if (!c->have_data || c->D != ref->D) return fail(GP_ERR_ARG, "constraint %d: D differs from the scored handle's", k);
        if (c->device != ref->device || c->s != ref->s) return fail(GP_ERR_ARG, "constraint %d lives on another device", k);
        if (c->P != 1) return fail(GP_ERR_ARG, "constraint %d: a constraint model needs P == 1", k);
        if (c->warp.n > 0) return fail(GP_ERR_ARG, "constraint %d: an output-warped model is no constraint model", k);
        if (c->sp.fitted || c->ens.S > 0)
            return fail(GP_ERR_ARG, "constraint %d: a handle with a sparse fit or an ensemble is no constraint model", k);
        if (!c->fitted) return fail(GP_ERR_STATE, "constraint %d: gp_fit first", k);
        if (!std::isfinite(bound[k]) || !std::isfinite(c_mean[k])) return fail(GP_ERR_ARG, "constraint %d: bound and c_mean must be finite", k);
        if (!(c_std[k] > 0.0) || !std::isfinite(c_std[k])) return fail(GP_ERR_ARG, "constraint %d: c_std must be positive and finite", k);
        in->c[k] = c;
    }
    in->K = K;
    in->bound = bound;
    in->c_mean = c_mean;
    in->c_std = c_std;
    return 0;
}

}   // namespace

// the table posterior of handle c over M locations already in its dXs: mean / var with noise and (grad) dDm / dDv, on the device
int table_posterior(gp_ctx *c, bool grad) {
    int rc;
    if ((rc = ensure_out(c))) return rc;
    if (grad && (rc = run_predict_grad(c))) return rc;
    if (!c->predicted || c->predicted_noise != 1)
        if ((rc = run_predict(c, 1))) return rc;
    return 0;
}

void feas_apply(gp_ctx *g, bool pof, double *acq) { launch_feas_apply(g->s, g->feas.dTabLogF, g->M, pof ? 1 : 0, acq); }

extern "C" int gp_feas_table(gp_t *g, gp_t *const *cons, int K, const double *bound, const double *c_mean, const double *c_std) {
    if (!g) return fail(GP_ERR_ARG, "null gp");
    GP_DEAD_CHECK(g);
    if (K == 0) {   // clear
        g->feas.K = 0;
        return 0;
    }
    if (!g->have_data) return fail(GP_ERR_STATE, "gp_set_data first");
    if (g->M < 1) return fail(GP_ERR_STATE, "gp_set_candidates first");
    FeasIn in;
    int rc;
    if ((rc = check_cons(g, cons, K, bound, c_mean, c_std, &in))) return rc;
    HIPCHK(hipSetDevice(g->device));
    const long M = g->M;
    const int D = g->D;
    g->feas.K = 0;
    if ((rc = g->feas.dTabLogF.reserve(M))) return rc;
    for (int k = 0; k < K; ++k) {
        gp_ctx *c = in.c[k];
        GP_SYNC(c->s);   // nothing on the stream still reads the table that is about to go
        if ((rc = c->dXs.reserve(M * D))) return rc;
        HIPCHK(hipMemcpyAsync(c->dXs, g->dXs, sizeof(double) * M * D, hipMemcpyDeviceToDevice, c->s));
        c->M = M;   // what gp_set_candidates leaves behind
        c->predicted = false;
        if (c->cost_tab == 1) c->cost_tab = 0;
        c->feas.K = 0;
        if ((rc = table_posterior(c, false))) return rc;
        launch_feas_table(c->s, c->dMean, c->dVar, M, c_mean[k], c_std[k], bound[k], k == 0, g->feas.dTabLogF);
    }
    GP_SYNC(g->s);
    g->feas.K = K;
    g->feas.M = M;
    return 0;
}

extern "C" int gp_feas_info(gp_t *g, int *K, int64_t *M) {
    if (!g || !K || !M) return fail(GP_ERR_ARG, "null argument");
    GP_DEAD_CHECK(g);
    *K = g->feas.K;
    *M = g->feas.K ? g->feas.M : 0;
    return 0;
}

extern "C" int gp_feas_get_table(gp_t *g, double *logF) {
    if (!g || !logF) return fail(GP_ERR_ARG, "null argument");
    GP_DEAD_CHECK(g);
    if (g->feas.K < 1) return fail(GP_ERR_STATE, "gp_feas_table first");
    HIPCHK(hipSetDevice(g->device));
    HIPCHK(hipMemcpyAsync(logF, g->feas.dTabLogF, sizeof(double) * g->feas.M, hipMemcpyDeviceToHost, g->s));
    GP_SYNC(g->s);
    return 0;
}

// A rows call: g null: log F (and its gradient) of the constraints alone; g given: the acquisition a of g times F.  Which handles
// take the fused route is decided once per call.  Handles on the fused route run passes into their pinned blocks; the others go
// through their table posterior over a whole group first (feas_fallback_tables) and are folded from their device buffers.
struct FeasCall {
    gp_ctx *g;
    const AcqSpec *a;
    const FeasIn &in;
    bool grad, g_fused, c_fused[GP_FEAS_MAX];
    int rule() const { return g ? acq_base(a->type & ~GP_ACQ_TIMES_FEAS) : 0; }
    bool pof() const { return g && rule() == GP_ACQ_POF; }
    bool per_cost() const { return g && acq_per_cost(a->type); }
    int base_rule() const { return pof() ? GP_ACQ_EI : rule(); }   // (pof: the fold overwrites the rule's score)
    bool any_fused() const {
        bool any = g && g_fused;
        for (int k = 0; k < in.K; ++k) any = any || c_fused[k];
        return any;
    }
};

// The handles OFF the fused route, over the mg locations of a group: the locations become their resident candidates, a constraint
// handle's posterior (with grad its gradients) and the scored handle's base scores stay in their table buffers, not drained.
// The handles ON it are made ready (inverse factor, scratch: everything that may synchronise, ahead of the first pass).
static int feas_fallback_tables(const FeasCall &fc, const double *Xs, int mg) {
    int rc;
    for (int k = 0; k < fc.in.K; ++k) {
        gp_ctx *c = fc.in.c[k];
        if (fc.c_fused[k]) {
            if ((rc = rows_prepare(c))) return rc;
            continue;
        }
        ++c->rows_fallback_calls;
        if ((rc = gp_set_candidates(c, Xs, mg))) return rc;
        if ((rc = table_posterior(c, fc.grad))) return rc;
    }
    gp_ctx *g = fc.g;
    if (!g) return fc.in.c[0]->pass.ready(fc.in.c[0]->s);   // the constraints alone report through the first handle's pinned block
    if (fc.g_fused) return rows_prepare(g);
    ++g->rows_fallback_calls;
    if ((rc = gp_set_candidates(g, Xs, mg))) return rc;
    const AcqSpec base{fc.base_rule(), fc.a->par, fc.a->fmin, fc.a->y_mean, fc.a->y_std};
    return run_acq(g, base, nullptr, fc.grad);
}

// where constraint k's posterior of the pass's locations lies: its pinned block rk[k].out ([mean][var][acq][dmdx][dvdx][dacq] for MV
// locations), or rows m0 .. of its table buffers
static FeasRows feas_sources(const FeasCall &fc, const PassReport *rk, int MV, int m0) {
    const int D = fc.in.c[0]->D;
    FeasRows fr{};
    fr.K = fc.in.K;
    for (int k = 0; k < fc.in.K; ++k) {
        const gp_ctx *c = fc.in.c[k];
        fr.bound[k] = fc.in.bound[k];
        fr.c_mean[k] = fc.in.c_mean[k];
        fr.c_std[k] = fc.in.c_std[k];
        if (fc.c_fused[k]) {
            const double *o = rk[k].out;
            fr.mean[k] = o;
            fr.var[k] = o + MV;
            fr.dm[k] = o + 3 * MV;
            fr.dv[k] = o + 3 * MV + (long)MV * D;
        } else {
            fr.mean[k] = c->dMean + m0;
            fr.var[k] = c->dVar + m0;
            fr.dm[k] = fc.grad ? c->dDm + (long)m0 * D : nullptr;
            fr.dv[k] = fc.grad ? c->dDv + (long)m0 * D : nullptr;
        }
    }
    return fr;
}

// One pass over locations [m0, m0 + mc) of a group: every fused handle's launch, the fold, the cost, then the owners' waits -- the
// first drains the shared stream, the others find it drained.  The fold's destination: the scored handle's pinned block (fused), its
// table scores dAcq / dDacq (fallback; drained by the group), or -- the constraints alone -- the acq / dacq slots of the first
// constraint handle's pinned block.
static int feas_pass(const FeasCall &fc, const double *Xs, int m0, int mc, double *out, double *dout) {
    gp_ctx *g = fc.g, *c0 = fc.in.c[0];
    hipStream_t s = c0->s;
    const int D = c0->D, MV = rows_layout(mc);
    const bool any = fc.any_fused(), scored_fused = g && fc.g_fused;
    RowsX rx;
    rx.M = mc;
    if (any) memcpy(rx.xs, Xs + (long)m0 * D, sizeof(double) * mc * D);   // (a fused handle: mc D <= ROWS_MAX_XS, rows_fused_ok)
    PassReport rg{}, rk[GP_FEAS_MAX];
    unsigned ag = 0, ak[GP_FEAS_MAX];
    if (scored_fused) {
        const RowsAcq aq{1, fc.base_rule(), fc.a->par, fc.a->fmin, fc.a->y_mean, fc.a->y_std, 0, 0, 0, nullptr, nullptr, nullptr};
        rows_enqueue(g, rx, 1, fc.grad, aq, &rg, &ag);   // with_noise=True, gpmodel.py:102
    }
    for (int k = 0; k < fc.in.K; ++k)
        if (fc.c_fused[k]) rows_enqueue(fc.in.c[k], rx, 1, fc.grad, RowsAcq{}, &rk[k], &ak[k]);
    const FeasRows fr = feas_sources(fc, rk, MV, m0);
    double *blk = g ? (scored_fused ? rg.out : nullptr) : c0->pass.block;
    if (!g) {
        launch_feas_rows(s, fr, mc, D, fc.grad, 0, nullptr, nullptr, blk + 2 * MV, blk + 3 * MV + 2L * MV * D);
    } else if (scored_fused) {
        launch_feas_rows(s, fr, mc, D, fc.grad, fc.pof(), blk + 2 * MV, blk + 3 * MV + 2L * MV * D, nullptr, nullptr);
        if (fc.per_cost()) cost_divide_block(g, rx, fc.grad, blk, MV);   // feasibility first, then the cost
    } else {
        launch_feas_rows(s, fr, mc, D, fc.grad, fc.pof(), g->dAcq + m0, fc.grad ? g->dDacq + (long)m0 * D : nullptr, nullptr, nullptr);
    }
    // every owner's wait is owed its arrivals, whatever an earlier one reports
    int rc = 0;
    if (scored_fused) rc = g->pass.wait(s, rg, ag, 0);
    for (int k = 0; k < fc.in.K; ++k)
        if (fc.c_fused[k]) {
            const int rck = fc.in.c[k]->pass.wait(s, rk[k], ak[k], 0);
            if (!rc) rc = rck;
        }
    if (rc) return rc;
    if (!any) GP_SYNC(s);
    if (blk) rows_unpack(blk, MV, m0, mc, D, nullptr, nullptr, out, nullptr, nullptr, fc.grad ? dout : nullptr);
    return 0;
}

// One group of mg <= ROWS_WIDE_M locations: the fallback handles' tables, then passes of `width` locations
static int feas_group(const FeasCall &fc, const double *Xs, int mg, double *out, double *dout) {
    gp_ctx *g = fc.g;
    const int D = fc.in.c[0]->D;
    int rc;
    if ((rc = feas_fallback_tables(fc, Xs, mg))) return rc;
    bool wide_ok = !g || !fc.g_fused || g->rows_wide;
    for (int k = 0; k < fc.in.K; ++k) wide_ok = wide_ok && (!fc.c_fused[k] || fc.in.c[k]->rows_wide);
    const int width = !fc.any_fused() ? mg : mg <= ROWS_MAX_M ? mg : (wide_ok && (long)mg * D <= ROWS_MAX_XS) ? mg : ROWS_MAX_M;
    for (int m0 = 0; m0 < mg; m0 += width)
        if ((rc = feas_pass(fc, Xs, m0, std::min(width, mg - m0), out, dout))) return rc;
    if (g && fc.g_fused) ++g->rows_fused_calls;
    for (int k = 0; k < fc.in.K; ++k)
        if (fc.c_fused[k]) ++fc.in.c[k]->rows_fused_calls;
    if (g && !fc.g_fused) {   // the scored handle's table scores, folded in place: the cost, then the drained copies
        if (fc.per_cost() && (rc = cost_divide(g, g->dXs, mg, fc.grad, g->dAcq, g->dDacq))) return rc;
        return scores_out(g, g->dAcq, g->dDacq, mg, D, out, fc.grad ? dout : nullptr);
    }
    return 0;
}

// groups of up to ROWS_WIDE_M locations; which handles take the fused route is decided once per call
static int feas_rows_call(gp_ctx *g, const AcqSpec *a, const FeasIn &in, const double *Xs, int64_t M, double *out, double *dout) {
    const int D = in.c[0]->D;
    FeasCall fc{g, a, in, dout != nullptr, false, {}};
    const int64_t mg_max = std::min<int64_t>(M, ROWS_WIDE_M);
    if (g) fc.g_fused = rows_take_fused(g, mg_max);
    for (int k = 0; k < in.K; ++k) fc.c_fused[k] = rows_take_fused(in.c[k], mg_max);
    int rc;
    for (int64_t m0 = 0; m0 < M; m0 += ROWS_WIDE_M) {
        const int mg = (int)std::min<int64_t>(ROWS_WIDE_M, M - m0);
        if ((rc = feas_group(fc, Xs + m0 * D, mg, out + m0, dout ? dout + m0 * D : nullptr))) return rc;
    }
    return 0;
}

extern "C" int gp_feas_rows(gp_t *const *cons, int K, const double *bound, const double *c_mean, const double *c_std,
                            const double *Xs, int64_t M, double *logF, double *dlogF) {
    if (!Xs || !logF) return fail(GP_ERR_ARG, "null argument");
    FeasIn in;
    int rc;
    if ((rc = check_cons(nullptr, cons, K, bound, c_mean, c_std, &in))) return rc;
    if (M < 1) return fail(GP_ERR_ARG, "M < 1");
    HIPCHK(hipSetDevice(in.c[0]->device));
    return feas_rows_call(nullptr, nullptr, in, Xs, M, logF, dlogF);
}

extern "C" int gp_acq_rows_feas(gp_t *g, gp_t *const *cons, int K, const double *bound, const double *c_mean, const double *c_std,
                                const double *Xs, int64_t M, int type, double par, double fmin, double y_mean, double y_std,
                                double *out, double *dout) {
    if (!g || !Xs || !out) return fail(GP_ERR_ARG, "null argument");
    GP_FITTED(g);
    if (M < 1) return fail(GP_ERR_ARG, "M < 1");
    if (g->P != 1) return fail(GP_ERR_ARG, "acquisitions need P == 1");
    const AcqSpec a{type, par, fmin, y_mean, y_std};
    const int rule = acq_base(type & ~GP_ACQ_TIMES_FEAS);
    if (rule < GP_ACQ_EI || rule > GP_ACQ_POF) return fail(GP_ERR_ARG, "unknown acquisition %d", type);
    if (rule == GP_ACQ_LCB) return fail(GP_ERR_ARG, "gp_acq_rows_feas: LCB takes no probability of feasibility");
    int rc;
    if ((rc = check_per_cost(g, type & ~GP_ACQ_TIMES_FEAS, false))) return rc;
    FeasIn in;
    if ((rc = check_cons(g, cons, K, bound, c_mean, c_std, &in))) return rc;
    return feas_rows_call(g, &a, in, Xs, M, out, dout);
}

extern "C" int gp_fmin_rows(gp_t *g, const int64_t *rows, int64_t n, double *fmin) {
    if (!g || !rows || !fmin) return fail(GP_ERR_ARG, "null argument");
    GP_FITTED(g);
    GP_NO_LAPLACE(g, "gp_fmin_rows");   // (before anything is copied: train_values would refuse after the rows went up)
    if (g->P != 1) return fail(GP_ERR_ARG, "gp_fmin_rows needs P == 1");
    if (n < 1) return fail(GP_ERR_ARG, "n < 1");
    for (int64_t i = 0; i < n; ++i)
        if (rows[i] < 0 || rows[i] >= g->N) return fail(GP_ERR_ARG, "training row out of range");
    int rc;
    if ((rc = g->feas.dWork.reserve(2 * n))) return rc;
    long long *dr = (long long *)g->feas.dWork.p;
    double *dv = g->feas.dWork + n;
    static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(long long) == sizeof(double), "rows travel as 8 bytes");
    HIPCHK(hipMemcpyAsync(dr, rows, sizeof(long long) * n, hipMemcpyHostToDevice, g->s));
    if ((rc = train_values(g))) return rc;
    launch_feas_gather(g->s, g->dMu, dr, n, dv);
    return argbest_read(g, dv, n, -1, nullptr, fmin);
}
