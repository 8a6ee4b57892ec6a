// Joint expected improvement (include/gphip.h, gp_qei_*; kernels: csrc/qei.hip): q <= 8 locations by value, scored as ONE batch over
// resident base samples.  A call is the fused rows path's passes over the inverse factor -- one forward launch for all q locations,
// for a gradient one backward launch -- with three kernels of its own between and behind them; it reports through the exact
// model's pass owner (one pinned block, one ticket) and moves none of the rows entries' counters.
#include "api_internal.h"

static_assert(GP_QEI_MAX_S == QEI_MAX_S && GP_QEI_MAX_Q == ROWS_WIDE_M, "the kernels take GP_QEI_MAX_S samples of GP_QEI_MAX_Q columns");
static_assert(QEI_OUT_GRAD + ROWS_MAX_XS <= ROWS_OUT_DOUBLES, "value, posterior and gradient fit the pinned block");

extern "C" int gp_qei_set(gp_t *g, const double *Z, int S, int q) {
    if (!g || !Z) return fail(GP_ERR_ARG, "null argument");
    GP_DEAD_CHECK(g);
    if (S < 1 || S > GP_QEI_MAX_S) return fail(GP_ERR_ARG, "gp_qei_set: S out of range (1..%d)", GP_QEI_MAX_S);
    if (q < 1 || q > GP_QEI_MAX_Q) return fail(GP_ERR_ARG, "gp_qei_set: q out of range (1..%d)", GP_QEI_MAX_Q);
    for (size_t i = 0; i < (size_t)S * q; ++i)
        if (!std::isfinite(Z[i])) return fail(GP_ERR_ARG, "gp_qei_set: a base sample is not finite");
    HIPCHK(hipSetDevice(g->device));
    QeiState &st = g->qei;
    GP_SYNC(g->s);   // nothing on the stream still reads the samples that are about to go
    st.S = st.q = 0;
    int rc;
    if ((rc = st.dZ.reserve((long)GP_QEI_MAX_S * GP_QEI_MAX_Q))) return rc;
    if (!st.dState) {
        if ((rc = st.dState.reserve(QEI_STATE_DOUBLES))) return rc;
        HIPCHK(hipMemsetAsync(st.dState, 0, sizeof(double) * QEI_STATE_DOUBLES, g->s));
    }
    std::vector<double> zt((size_t)S * q);   // column-major on the device: the joint step's threads walk a column side by side
    for (int s = 0; s < S; ++s)
        for (int l = 0; l < q; ++l) zt[(size_t)l * S + s] = Z[(size_t)s * q + l];
    HIPCHK(hipMemcpyAsync(st.dZ, zt.data(), sizeof(double) * zt.size(), hipMemcpyHostToDevice, g->s));
    GP_SYNC(g->s);   // the copy above is the call's own: it goes out of scope here
    st.S = S;
    st.q = q;
    return 0;
}

extern "C" int gp_qei_info(gp_t *g, int *S, int *q) {
    if (!g || !S || !q) return fail(GP_ERR_ARG, "null argument");
    *S = g->qei.S;
    *q = g->qei.S ? g->qei.q : 0;
    return 0;
}

extern "C" int gp_qei_stats(gp_t *g, int64_t *calls, int64_t *grad_calls) {
    if (!g) return fail(GP_ERR_ARG, "null gp");
    if (calls) *calls = g->qei.calls;
    if (grad_calls) *grad_calls = g->qei.grad_calls;
    return 0;
}

extern "C" int gp_qei_rows(gp_t *g, const double *Xq, int q, int include_noise, double par, double fmin, double y_mean, double y_std,
                           double *out, double *dout, double *mean, double *cov) {
    if (!g || !Xq || !out) return fail(GP_ERR_ARG, "null argument");
    GP_FITTED(g);
    GP_NO_LAPLACE(g, "gp_qei_rows");
    QeiState &st = g->qei;
    if (st.S < 1) return fail(GP_ERR_STATE, "gp_qei_rows: no base samples are resident (gp_qei_set)");
    if (g->P != 1) return fail(GP_ERR_STATE, "gp_qei_rows needs P == 1");
    if (g->kp.gower) return fail(GP_ERR_STATE, "gp_qei_rows: not available for a Gower kernel");
    if (g->warp.n > 0) return fail(GP_ERR_STATE, "gp_qei_rows: not available while an output warp is on");
    GP_NO_MEAN(g, "gp_qei_rows");
    const int D = g->D;
    if (q < 1 || q > st.q) return fail(GP_ERR_ARG, "gp_qei_rows: q out of range (1..%d, the resident samples' columns)", st.q);
    if ((long)q * D > ROWS_MAX_XS)
        return fail(GP_ERR_ARG, "gp_qei_rows: q * D = %ld coordinates, the kernel arguments take %d", (long)q * D, ROWS_MAX_XS);
    for (int i = 0; i < q * D; ++i)
        if (!std::isfinite(Xq[i])) return fail(GP_ERR_ARG, "gp_qei_rows: a location is not finite");
    if (!std::isfinite(par) || !std::isfinite(fmin) || !std::isfinite(y_mean))
        return fail(GP_ERR_ARG, "gp_qei_rows: par, fmin and y_mean must be finite");
    if (!(y_std > 0.0) || !std::isfinite(y_std)) return fail(GP_ERR_ARG, "gp_qei_rows: y_std must be positive and finite");
    int rc;
    if ((rc = ensure_linv(g))) return rc;   // true fp64 in either arithmetic mode; a call always needs the factor: built at the first one
    RowsWork w;
    if ((rc = rows_scratch(g, &w))) return rc;
    const int want_grad = dout != nullptr;
    const int nt_loads = g->rows_nt < 0 ? (g->Npad > 8192 ? 1 : 0) : g->rows_nt;
    const double N2 = (double)g->N * g->N;
    RowsX rx;
    rx.M = q;
    memcpy(rx.xs, Xq, sizeof(double) * q * D);
    const QeiArgs qa{st.dZ.p, st.S, st.S, par, fmin, y_mean, y_std};
    const PassReport r = g->pass.next();
    const bool timed = g->profiling;
    if (timed) g->nphases = 0;
    hipStream_t s = g->s;
    int ph = timed ? phase_begin(g, "qei_forward", N2 * q, 4.0 * N2) : -1;
    launch_rows_forward(s, g->dLi, g->Npad, rx, g->kp, g->dX, g->N, g->dAlpha, w, nt_loads);
    if (timed) phase_end(g, ph);
    ph = timed ? phase_begin(g, "qei_gram", (double)g->N * q * (q + 1), 0.0) : -1;
    launch_qei_gram(s, q, g->N, g->Npad, w);
    if (timed) phase_end(g, ph);
    ph = timed ? phase_begin(g, "qei_joint", (double)st.S * q * q, 0.0) : -1;
    launch_qei_joint(s, rx, g->kp, g->N, g->Npad, w, g->kp.variance, include_noise ? g->noise : 0.0, qa, want_grad, st.dState, r);
    if (timed) phase_end(g, ph);
    if (want_grad) {
        ph = timed ? phase_begin(g, "qei_backward", N2 * q, 4.0 * N2) : -1;
        launch_rows_backward(s, g->dLi, g->Npad, q, w, nt_loads);
        if (timed) phase_end(g, ph);
        ph = timed ? phase_begin(g, "qei_close", 2.0 * g->N * q * (q + D), 0.0) : -1;
        launch_qei_close(s, rx, g->kp, g->dX, g->N, g->Npad, g->dAlpha, w, st.dState, r);
        if (timed) phase_end(g, ph);
    }
    if ((rc = g->pass.wait(s, r, want_grad ? rows_finish_grid(g->N) : 0u, 0u))) return rc;
    ++st.calls;
    if (want_grad) ++st.grad_calls;
    const double *o = g->pass.block;
    if (o[QEI_OUT_STATUS] != 0.0) return (int)o[QEI_OUT_STATUS];   // the 1-based row of the pivot that failed: nothing is written
    out[0] = o[QEI_OUT_VALUE];
    if (dout) memcpy(dout, o + QEI_OUT_GRAD, sizeof(double) * q * D);
    if (mean) memcpy(mean, o + QEI_OUT_MEAN, sizeof(double) * q);
    if (cov) memcpy(cov, o + QEI_OUT_COV, sizeof(double) * q * q);
    return 0;
}
