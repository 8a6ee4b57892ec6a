// Multi-objective: expected hypervolume improvement of K = 2 or 3 independent objective GPs (Emmerich et al. 2011; Yang et al.
// 2019).  Every objective stays a live handle with its factor -- EHVI needs each one's variance --; the SCORED handle, objective
// 0, owns the cell decomposition (EhviState) and receives the scores.  The handles of a call live on one device, so they share one
// stream set (DevStreams): they are sequenced on that stream, folded by one kernel (ehvi.hip) and drained once, as the black-box
// constraints are (api_feas.hip).
#include "api_internal.h"

namespace {
struct EhviIn {
    int K;
    gp_ctx *h[GP_EHVI_MAX_OBJ];   // h[0]: the scored handle
    const double *y_mean, *y_std;
};

// the objectives of a call: the scored handle's state, and each other handle against the device, stream and width they share
int check_objs(gp_ctx *g, gp_t *const *others, int K, const double *y_mean, const double *y_std, EhviIn *in) {
    if (g->ehvi.K < 1) return fail(GP_ERR_STATE, "gp_ehvi_set first");
    if (K != g->ehvi.K) return fail(GP_ERR_ARG, "K = %d objectives, the resident decomposition has %d", K, g->ehvi.K);
    if (!others || !y_mean || !y_std) return fail(GP_ERR_ARG, "null argument");
    in->h[0] = g;
    for (int k = 1; k < K; ++k) {
        gp_ctx *c = others[k - 1];
        if (!c) return fail(GP_ERR_ARG, "null objective handle (%d)", k);
        GP_DEAD_CHECK(c);
        if (c == g) return fail(GP_ERR_ARG, "objective %d is the scored handle itself", k);
        for (int j = 1; j < k; ++j)
            if (in->h[j] == c) return fail(GP_ERR_ARG, "objective handle %d is listed twice", k);
        if (!c->have_data || c->D != g->D) return fail(GP_ERR_ARG, "objective %d: D differs from the scored handle's", k);
        if (c->device != g->device || c->s != g->s) return fail(GP_ERR_ARG, "objective %d lives on another device", k);
        in->h[k] = c;
    }
    for (int k = 0; k < K; ++k) {
        const gp_ctx *c = in->h[k];
        if (c->P != 1) return fail(GP_ERR_ARG, "objective %d: an objective model needs P == 1", k);
        if (c->warp.n > 0) return fail(GP_ERR_ARG, "objective %d: an output-warped model is no objective model", k);
        if (c->sp.fitted || c->ens.S > 0)
            return fail(GP_ERR_ARG, "objective %d: a handle with a sparse fit or an ensemble is no objective model", k);
        if (!c->fitted) return fail(GP_ERR_STATE, "objective %d: gp_fit first", k);
        if (!std::isfinite(y_mean[k])) return fail(GP_ERR_ARG, "objective %d: y_mean must be finite", k);
        if (!(y_std[k] > 0.0) || !std::isfinite(y_std[k])) return fail(GP_ERR_ARG, "objective %d: y_std must be positive and finite", k);
    }
    in->K = K;
    in->y_mean = y_mean;
    in->y_std = y_std;
    return 0;
}

EhviCells ehvi_cells(const gp_ctx *g) {
    const EhviState &e = g->ehvi;
    EhviCells ec{};
    ec.K = e.K;
    ec.C = e.C;
    for (int k = 0; k < e.K; ++k) {
        ec.L[k] = e.L[k];
        ec.off[k] = e.off[k];
    }
    ec.levels = e.dLevels;
    ec.cells = e.dCells;
    return ec;
}

// -EHVI over the scored handle's resident candidates into its dAcq, not drained: the table to the other handles device to device,
// K table posteriors, one launch
int ehvi_table_scores(const EhviIn &in) {
    gp_ctx *g = in.h[0];
    const long M = g->M;
    const int D = g->D;
    int rc;
    EhviRows er{};
    for (int k = 0; k < in.K; ++k) {
        gp_ctx *c = in.h[k];
        if (k > 0) {
            GP_SYNC(c->s);   // nothing on the stream still reads the table that is about to go
            if ((rc = c->dXs.reserve(M * D))) return rc;
            HIPCHK(hipMemcpyAsync(c->dXs, g->dXs, sizeof(double) * M * D, hipMemcpyDeviceToDevice, c->s));
            c->M = M;   // what gp_set_candidates leaves behind
            c->predicted = false;
            if (c->cost_tab == 1) c->cost_tab = 0;
            c->feas.K = 0;
        }
        if ((rc = table_posterior(c, false))) return rc;
        er.mean[k] = c->dMean;
        er.var[k] = c->dVar;
        er.y_mean[k] = in.y_mean[k];
        er.y_std[k] = in.y_std[k];
    }
    launch_ehvi_table(g->s, ehvi_cells(g), er, M, g->dAcq);
    return 0;
}

// the preamble of the three table entries
int ehvi_table_call(gp_ctx *g, gp_t *const *others, int K, const double *y_mean, const double *y_std, EhviIn *in) {
    if (!g) return fail(GP_ERR_ARG, "null gp");
    GP_DEAD_CHECK(g);
    int rc;
    if ((rc = check_objs(g, others, K, y_mean, y_std, in))) return rc;
    if (g->M < 1) return fail(GP_ERR_STATE, "gp_set_candidates first");
    HIPCHK(hipSetDevice(g->device));
    return 0;
}
}   // namespace

extern "C" int gp_ehvi_set(gp_t *g, int K, const double *levels, const int *nlev, const int *cell_lo, const int *cell_hi, int C) {
    if (!g) return fail(GP_ERR_ARG, "null gp");
    GP_DEAD_CHECK(g);
    if (K == 0) {   // clear
        g->ehvi.K = g->ehvi.C = 0;
        return 0;
    }
    if (K < 2 || K > GP_EHVI_MAX_OBJ) return fail(GP_ERR_ARG, "K out of range (2..%d objectives)", GP_EHVI_MAX_OBJ);
    if (!levels || !nlev || !cell_lo || !cell_hi) return fail(GP_ERR_ARG, "null argument");
    if (C < 1 || C > GP_EHVI_MAX_CELLS) return fail(GP_ERR_ARG, "C out of range (1..%d cells)", GP_EHVI_MAX_CELLS);
    int off[GP_EHVI_MAX_OBJ], total = 0;
    for (int k = 0; k < K; ++k) {
        if (nlev[k] < 2 || nlev[k] > GP_EHVI_MAX_LEVELS)
            return fail(GP_ERR_ARG, "objective %d: %d levels, out of range (2..%d)", k, nlev[k], GP_EHVI_MAX_LEVELS);
        off[k] = total;
        total += nlev[k];
    }
    std::vector<double> lv(levels, levels + total);
    for (int k = 0; k < K; ++k) {
        lv[off[k]] = -INFINITY;   // index 0 IS -inf
        for (int i = 1; i < nlev[k]; ++i) {
            const double v = lv[off[k] + i];
            if (!std::isfinite(v)) return fail(GP_ERR_ARG, "objective %d: level %d is not finite", k, i);
            if (i > 1 && !(v > lv[off[k] + i - 1])) return fail(GP_ERR_ARG, "objective %d: the levels must increase (level %d)", k, i);
        }
    }
    std::vector<unsigned int> cells((size_t)C * K);
    for (long c = 0; c < C; ++c)
        for (int k = 0; k < K; ++k) {
            const int lo = cell_lo[c * K + k], hi = cell_hi[c * K + k];
            if (lo < 0 || hi >= nlev[k] || lo >= hi)
                return fail(GP_ERR_ARG, "cell %ld, objective %d: indices (%d, %d) need 0 <= lo < hi < %d", c, k, lo, hi, nlev[k]);
            cells[c * K + k] = (unsigned int)lo | ((unsigned int)hi << 16);
        }
    HIPCHK(hipSetDevice(g->device));
    GP_SYNC(g->s);   // no launch still reads the decomposition that is about to go
    EhviState &e = g->ehvi;
    e.K = e.C = 0;
    int rc;
    if ((rc = e.dLevels.reserve(total))) return rc;
    if ((rc = e.dCells.reserve((long)C * K))) return rc;
    HIPCHK(hipMemcpyAsync(e.dLevels, lv.data(), sizeof(double) * total, hipMemcpyHostToDevice, g->s));
    HIPCHK(hipMemcpyAsync(e.dCells, cells.data(), sizeof(unsigned int) * cells.size(), hipMemcpyHostToDevice, g->s));
    GP_SYNC(g->s);   // (the host vectors go out of scope)
    for (int k = 0; k < K; ++k) {
        e.L[k] = nlev[k];
        e.off[k] = off[k];
    }
    e.K = K;
    e.C = C;
    return 0;
}

extern "C" int gp_ehvi_info(gp_t *g, int *K, int *C) {
    if (!g || !K || !C) return fail(GP_ERR_ARG, "null argument");
    GP_DEAD_CHECK(g);
    *K = g->ehvi.K;
    *C = g->ehvi.K ? g->ehvi.C : 0;
    return 0;
}

extern "C" int gp_ehvi_table(gp_t *g, gp_t *const *others, int K, const double *y_mean, const double *y_std, double *out) {
    EhviIn in;
    int rc;
    if ((rc = ehvi_table_call(g, others, K, y_mean, y_std, &in))) return rc;
    if ((rc = ehvi_table_scores(in))) return rc;
    return scores_out(g, g->dAcq, nullptr, g->M, g->D, out, nullptr);
}

extern "C" int gp_ehvi_argbest(gp_t *g, gp_t *const *others, int K, const double *y_mean, const double *y_std, int sense,
                               const int64_t *exclude, int nex, int64_t *idx, double *val) {
    if (!idx || !val) return fail(GP_ERR_ARG, "null argument");
    EhviIn in;
    int rc;
    if ((rc = ehvi_table_call(g, others, K, y_mean, y_std, &in))) return rc;
    if ((rc = check_sense(sense))) return rc;
    if ((rc = check_exclude(exclude, nex, g->M))) return rc;
    if ((rc = ehvi_table_scores(in))) return rc;
    return select_best(g, g->dAcq, g->M, sense, exclude, nex, idx, val);
}

extern "C" int gp_ehvi_topk(gp_t *g, gp_t *const *others, int K, const double *y_mean, const double *y_std, int sense, int k,
                            int64_t *idx, double *val) {
    if (!idx || !val) return fail(GP_ERR_ARG, "null argument");
    EhviIn in;
    int rc;
    if ((rc = ehvi_table_call(g, others, K, y_mean, y_std, &in))) return rc;
    if ((rc = check_sense(sense))) return rc;
    if ((rc = check_k(k))) return rc;
    if ((rc = ehvi_table_scores(in))) return rc;
    return select_topk(g, g->dAcq, g->M, sense, k, idx, val);
}

// A rows call.  Which handles take the fused route is decided once per call.  Handles on it run passes into their pinned blocks;
// the others go through their table posterior over a whole group first and are folded from their device buffers.  A fused pass
// is ALWAYS the gradient call's: a value-only pass sums |w|^2 in another order (rows_body.h), and the value is to have the same
// bits with and without dout -- a value-only call pays the backward launch for it (the optimiser's calls all carry a gradient).
// (The table posterior's mean and variance come from the same kernels either way.)
struct EhviCall {
    const EhviIn &in;
    bool grad, fused[GP_EHVI_MAX_OBJ];
    bool any_fused() const {
        bool any = false;
        for (int k = 0; k < in.K; ++k) any = any || fused[k];
        return any;
    }
};

// One pass over locations [m0, m0 + mc) of a group: every fused handle's launch, the fold, then the owners' waits -- the first
// drains the shared stream, the others find it drained.  The fold's destination: the acq / dacq slots of the scored handle's pinned
// block (fused), or its table scores dAcq / dDacq (fallback; drained by the group).
static int ehvi_pass(const EhviCall &ec, const double *Xs, int m0, int mc, double *out, double *dout) {
    gp_ctx *g = ec.in.h[0];
    hipStream_t s = g->s;
    const int D = g->D, MV = rows_layout(mc);
    const bool any = ec.any_fused();
    RowsX rx;
    rx.M = mc;
    if (any) memcpy(rx.xs, Xs + (long)m0 * D, sizeof(double) * mc * D);   // (a fused handle: mc D <= ROWS_MAX_XS, rows_fused_ok)
    PassReport rk[GP_EHVI_MAX_OBJ];
    unsigned ak[GP_EHVI_MAX_OBJ];
    EhviRows er{};
    for (int k = 0; k < ec.in.K; ++k) {
        gp_ctx *c = ec.in.h[k];
        er.y_mean[k] = ec.in.y_mean[k];
        er.y_std[k] = ec.in.y_std[k];
        if (ec.fused[k]) {
            rows_enqueue(c, rx, 1, 1, RowsAcq{}, &rk[k], &ak[k]);   // with_noise=True, gpmodel.py:102; always the gradient pass (EhviCall)
            const double *o = rk[k].out;
            er.mean[k] = o;
            er.var[k] = o + MV;
            er.dm[k] = o + 3 * MV;
            er.dv[k] = o + 3 * MV + (long)MV * D;
        } else {
            er.mean[k] = c->dMean + m0;
            er.var[k] = c->dVar + m0;
            er.dm[k] = ec.grad ? c->dDm + (long)m0 * D : nullptr;
            er.dv[k] = ec.grad ? c->dDv + (long)m0 * D : nullptr;
        }
    }
    double *blk = ec.fused[0] ? rk[0].out : nullptr;
    if (blk)
        launch_ehvi_rows(s, ehvi_cells(g), er, mc, D, ec.grad, blk + 2 * MV, blk + 3 * MV + 2L * MV * D);
    else
        launch_ehvi_rows(s, ehvi_cells(g), er, mc, D, ec.grad, g->dAcq + m0, ec.grad ? g->dDacq + (long)m0 * D : nullptr);
    // every owner's wait is owed its arrivals, whatever an earlier one reports
    int rc = 0;
    for (int k = 0; k < ec.in.K; ++k)
        if (ec.fused[k]) {
            const int rck = ec.in.h[k]->pass.wait(s, rk[k], ak[k], 0);
            if (!rc) rc = rck;
        }
    if (rc) return rc;
    if (!any) GP_SYNC(s);
    if (blk) rows_unpack(blk, MV, m0, mc, D, nullptr, nullptr, out, nullptr, nullptr, ec.grad ? dout : nullptr);
    return 0;
}

// One group of mg <= ROWS_WIDE_M locations: the fallback handles' tables (the fused ones made ready: everything that may
// synchronise, ahead of the first pass), then passes of `width` locations
static int ehvi_group(const EhviCall &ec, const double *Xs, int mg, double *out, double *dout) {
    gp_ctx *g = ec.in.h[0];
    const int D = g->D;
    int rc;
    bool wide_ok = true;
    for (int k = 0; k < ec.in.K; ++k) {
        gp_ctx *c = ec.in.h[k];
        if (ec.fused[k]) {
            if ((rc = rows_prepare(c))) return rc;
            wide_ok = wide_ok && c->rows_wide;
            continue;
        }
        ++c->rows_fallback_calls;
        if ((rc = gp_set_candidates(c, Xs, mg))) return rc;
        if ((rc = table_posterior(c, ec.grad))) return rc;
    }
    const int width = !ec.any_fused() ? mg : mg <= ROWS_MAX_M ? mg : (wide_ok && (long)mg * D <= ROWS_MAX_XS) ? mg : ROWS_MAX_M;
    for (int m0 = 0; m0 < mg; m0 += width)
        if ((rc = ehvi_pass(ec, Xs, m0, std::min(width, mg - m0), out, dout))) return rc;
    for (int k = 0; k < ec.in.K; ++k)
        if (ec.fused[k]) ++ec.in.h[k]->rows_fused_calls;
    if (!ec.fused[0]) return scores_out(g, g->dAcq, g->dDacq, mg, D, out, ec.grad ? dout : nullptr);
    return 0;
}

extern "C" int gp_ehvi_rows(gp_t *g, gp_t *const *others, int K, const double *y_mean, const double *y_std, const double *Xs,
                            int64_t M, double *out, double *dout) {
    if (!g || !Xs || !out) return fail(GP_ERR_ARG, "null argument");
    GP_DEAD_CHECK(g);
    EhviIn in;
    int rc;
    if ((rc = check_objs(g, others, K, y_mean, y_std, &in))) return rc;
    if (M < 1) return fail(GP_ERR_ARG, "M < 1");
    HIPCHK(hipSetDevice(g->device));
    const int D = g->D;
    EhviCall ec{in, dout != nullptr, {}};
    const int64_t mg_max = std::min<int64_t>(M, ROWS_WIDE_M);
    for (int k = 0; k < K; ++k) ec.fused[k] = rows_take_fused(in.h[k], mg_max);
    for (int64_t m0 = 0; m0 < M; m0 += ROWS_WIDE_M) {
        const int mg = (int)std::min<int64_t>(ROWS_WIDE_M, M - m0);
        if ((rc = ehvi_group(ec, Xs + m0 * D, mg, out + m0, dout ? dout + m0 * D : nullptr))) return rc;
    }
    return 0;
}
