// The cost surface behind GP_ACQ_PER_COST: GPyOpt's CostModel with cost_withGradients = 'evaluation_time' (core/task/cost.py)
// divides EI and MPI by exp(m_c(x)), m_c the posterior mean of a second GP over the logarithm of the evaluation times
// (acquisitions/base.py:33-50).  The handle keeps a snapshot of that mean -- m_c(x) = shift + scale sum_j alpha_j k(x, Xc_j) -- and
// divides its scores on the device (csrc/cost.hip).
#include "api_internal.h"

static const int COST_FEW_ROWS = ROWS_WIDE_M;   // up to this many locations take the few-rows launch

extern "C" int gp_cost_set(gp_t *g, const double *Xc, int64_t Nc, const double *alpha, int kernel, int ard, double variance,
                           const double *lengthscale, double shift, double scale) {
    if (!g) return fail(GP_ERR_ARG, "null gp");
    GP_DEAD_CHECK(g);
    CostState &c = g->cost;
    if (Nc != 0) GP_NO_LAPLACE(g, "gp_cost_set");
    if (Nc == 0) {   // clear
        c.Nc = 0;
        g->cost_tab = 0;
        return 0;
    }
    if (Nc < 0) return fail(GP_ERR_ARG, "gp_cost_set: Nc < 0");
    if (!Xc || !alpha || !lengthscale) return fail(GP_ERR_ARG, "null argument");
    if (!g->have_data) return fail(GP_ERR_STATE, "gp_cost_set: gp_set_data first (the surface has the handle's D columns)");
    if (kernel < GP_KERNEL_RBF || kernel > GP_KERNEL_EXPONENTIAL) return fail(GP_ERR_ARG, "gp_cost_set: unknown kernel %d", kernel);
    if (!(variance > 0.0) || !std::isfinite(variance)) return fail(GP_ERR_ARG, "gp_cost_set: variance must be positive and finite");
    if (!std::isfinite(shift) || !std::isfinite(scale)) return fail(GP_ERR_ARG, "gp_cost_set: shift and scale must be finite");
    const int D = g->D;
    for (int d = 0; d < (ard ? D : 1); ++d)
        if (!(lengthscale[d] > 0.0) || !std::isfinite(lengthscale[d]))
            return fail(GP_ERR_ARG, "gp_cost_set: lengthscale must be positive and finite (entry %d)", d);
    HIPCHK(hipSetDevice(g->device));
    GP_SYNC(g->s);   // nothing on the stream still reads the surface that is about to go
    KernParams kp{};
    kp.kernel = kernel;
    kp.D = D;
    kp.variance = variance;
    for (int d = 0; d < GP_MAX_D; ++d) kp.ls[d] = d < D ? lengthscale[ard ? d : 0] : 1.0;
    const int ld = std::max(D, 8);
    std::vector<double> xs((size_t)Nc * ld, 0.0);   // Xc / lengthscale: the division the kernels apply to the locations
    for (int64_t j = 0; j < Nc; ++j)
        for (int d = 0; d < D; ++d) xs[(size_t)j * ld + d] = Xc[j * D + d] / kp.ls[d];
    c.Nc = 0;
    g->cost_tab = 0;
    int rc;
    if ((rc = c.dXcs.reserve((long)Nc * ld))) return rc;
    if ((rc = c.dAlpha.reserve((long)Nc))) return rc;
    HIPCHK(hipMemcpy(c.dXcs, xs.data(), sizeof(double) * Nc * ld, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c.dAlpha, alpha, sizeof(double) * Nc, hipMemcpyHostToDevice));
    c.kp = kp;
    c.ld = ld;
    c.shift = shift;
    c.scale = scale;
    c.Nc = (long)Nc;
    return 0;
}

extern "C" int gp_cost_info(gp_t *g, int64_t *Nc) {
    if (!g || !Nc) return fail(GP_ERR_ARG, "null argument");
    *Nc = g->cost.Nc;
    return 0;
}

// a few locations on the host: passes of as many as travel in the kernel arguments
template <class Each>
static void cost_rows_passes(int D, const double *Xs, int M, Each each) {
    const int width = std::max(1, std::min(COST_FEW_ROWS, ROWS_MAX_XS / D));
    for (int m0 = 0; m0 < M; m0 += width) {
        RowsX rx;
        rx.M = std::min(width, M - m0);
        memcpy(rx.xs, Xs + (long)m0 * D, sizeof(double) * rx.M * D);
        each(m0, rx);
    }
}

// the scratch of a values-only table launch that is cut along the surface (null where launch_cost_table would not cut it)
static int cost_part(gp_ctx *g, long M, double **part) {
    const long n = (long)cost_table_part_elems(M, g->cost.Nc, g->cost.kp.D);
    *part = nullptr;
    if (!n) return 0;
    int rc;
    if ((rc = g->cost.dPart.reserve(n))) return rc;
    *part = g->cost.dPart;
    return 0;
}

extern "C" int gp_cost_rows(gp_t *g, const double *Xs, int64_t M, double *logc, double *dlogc) {
    if (!g || !Xs || !logc) return fail(GP_ERR_ARG, "null argument");
    GP_DEAD_CHECK(g);
    CostState &c = g->cost;
    if (c.Nc < 1) return fail(GP_ERR_STATE, "gp_cost_set first");
    if (M < 1) return fail(GP_ERR_ARG, "M < 1");
    HIPCHK(hipSetDevice(g->device));
    const int D = c.kp.D;
    int rc;
    if ((rc = c.dWork.reserve((long)M * (2 * D + 1)))) return rc;
    double *dX = c.dWork, *dl = dX + M * D, *dd = dl + M;
    if (M <= COST_FEW_ROWS) {
        cost_rows_passes(D, Xs, (int)M, [&](int m0, const RowsX &rx) {
            launch_cost_rows(g->s, rx, c.dXcs, c.ld, c.dAlpha, c.Nc, c.kp, c.shift, c.scale, dlogc != nullptr, dl + m0,
                             dd + (long)m0 * D, nullptr, 0);
        });
    } else {
        HIPCHK(hipMemcpyAsync(dX, Xs, sizeof(double) * M * D, hipMemcpyHostToDevice, g->s));
        double *part = nullptr;
        if (!dlogc && (rc = cost_part(g, M, &part))) return rc;
        launch_cost_table(g->s, dX, M, c.dXcs, c.ld, c.dAlpha, c.Nc, c.kp, c.shift, c.scale, dl, dlogc ? dd : nullptr, part);
    }
    return scores_out(g, dl, dd, M, D, logc, dlogc);
}

int cost_divide(gp_ctx *g, const double *X, long M, bool grad, double *acq, double *dacq) {
    CostState &c = g->cost;
    const int D = g->D;
    const int tab = (X == g->dXs.p && M == g->M) ? 1 : (X == g->sp.dTab.p && M == g->sp.tM) ? 2 : 0;
    int rc;
    double *dl, *dd = nullptr;
    if (tab) {
        if (c.dTabLogc.cap < M) g->cost_tab = 0;   // (reserve does not keep the contents)
        if ((rc = c.dTabLogc.reserve(M))) return rc;
        dl = c.dTabLogc;
        if (grad) {
            if ((rc = c.dWork.reserve(M * D))) return rc;
            dd = c.dWork;
        }
    } else {
        if ((rc = c.dWork.reserve(M * (D + 1)))) return rc;
        dl = c.dWork;
        dd = dl + M;
    }
    // (with gradients the pass writes logc as well: the same bits, one summation order)
    if (grad || !tab || g->cost_tab != tab) {
        double *part = nullptr;
        if (!grad && (rc = cost_part(g, M, &part))) return rc;
        launch_cost_table(g->s, X, M, c.dXcs, c.ld, c.dAlpha, c.Nc, c.kp, c.shift, c.scale, dl, grad ? dd : nullptr, part);
        if (tab) g->cost_tab = tab;
    }
    launch_cost_apply(g->s, dl, grad ? dd : nullptr, M, D, acq, grad ? dacq : nullptr);
    return 0;
}

void cost_divide_block(gp_ctx *g, const RowsX &rx, bool grad, double *blk, int MV) {
    const CostState &c = g->cost;
    launch_cost_rows(g->s, rx, c.dXcs, c.ld, c.dAlpha, c.Nc, c.kp, c.shift, c.scale, grad ? 1 : 0, nullptr, nullptr, blk, MV);
}
