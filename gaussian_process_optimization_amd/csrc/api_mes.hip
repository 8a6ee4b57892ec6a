// Max-value entropy search (Wang & Jegelka, ICML 2017; mirrored for a minimum): the K samples of the minimum's value behind
// GP_ACQ_MES, and the two reductions over the resident candidates' posterior from which the caller draws them (csrc/mes.hip) --
// log S(y) = sum_i log Phi((m_i - y) / s_i) at up to GP_MES_MAX_G trial values, and a bracket for its quantiles.  The rule itself
// is mes_terms (acq_math.h), scored by the exact model's entries through check_acq / score_rows / rows_acq.
#include "api_internal.h"

static_assert(GP_MES_MAX_G == MES_MAX_G, "the kernels' argument takes GP_MES_MAX_G trial values");

extern "C" int gp_mes_set(gp_t *g, const double *ystar, int K) {
    if (!g) return fail(GP_ERR_ARG, "null gp");
    GP_DEAD_CHECK(g);
    if (K < 0 || K > GP_MES_MAX_K) return fail(GP_ERR_ARG, "gp_mes_set: K out of range (0..%d)", GP_MES_MAX_K);
    if (K == 0) {   // clear
        g->mes.K = 0;
        return 0;
    }
    GP_NO_LAPLACE(g, "gp_mes_set");
    if (!ystar) return fail(GP_ERR_ARG, "null argument");
    for (int k = 0; k < K; ++k)
        if (!std::isfinite(ystar[k])) return fail(GP_ERR_ARG, "gp_mes_set: sample %d is not finite", k);
    HIPCHK(hipSetDevice(g->device));
    GP_SYNC(g->s);   // nothing on the stream still reads the samples that are about to go
    int rc;
    g->mes.K = 0;
    if ((rc = g->mes.dY.reserve(GP_MES_MAX_K))) return rc;
    HIPCHK(hipMemcpy(g->mes.dY, ystar, sizeof(double) * K, hipMemcpyHostToDevice));
    g->mes.K = K;
    return 0;
}

extern "C" int gp_mes_info(gp_t *g, int *K) {
    if (!g || !K) return fail(GP_ERR_ARG, "null argument");
    *K = g->mes.K;
    return 0;
}

// the resident candidates' table posterior with the noise the caller asks for (the cache is keyed by it: run_acq, gp_predict_warped
// and gp_feas_table ask for theirs the same way), and the reductions' scratch
static int mes_table(gp_ctx *g, int include_noise, double y_std, const char *who) {
    GP_NO_LAPLACE(g, who);
    if (g->P != 1) return fail(GP_ERR_ARG, "%s needs P == 1", who);
    if (!(y_std > 0.0) || !std::isfinite(y_std)) return fail(GP_ERR_ARG, "%s: y_std must be positive and finite", who);
    int rc;
    if ((rc = ensure_out(g))) return rc;
    if (!g->predicted || g->predicted_noise != (include_noise ? 1 : 0))
        if ((rc = run_predict(g, include_noise ? 1 : 0))) return rc;
    return g->mes.dPart.reserve((long)mes_part_elems(g->M));
}

extern "C" int gp_mes_logsurv(gp_t *g, int include_noise, double y_mean, double y_std, const double *y, int G, double *out) {
    if (!g || !y || !out) return fail(GP_ERR_ARG, "null argument");
    GP_SCORING(g);
    if (G < 1 || G > GP_MES_MAX_G) return fail(GP_ERR_ARG, "gp_mes_logsurv: G out of range (1..%d)", GP_MES_MAX_G);
    if (!std::isfinite(y_mean)) return fail(GP_ERR_ARG, "gp_mes_logsurv: y_mean must be finite");
    MesY my;
    my.G = G;
    for (int i = 0; i < G; ++i) {
        if (!std::isfinite(y[i])) return fail(GP_ERR_ARG, "gp_mes_logsurv: trial value %d is not finite", i);
        my.y[i] = y[i];
    }
    for (int i = G; i < MES_MAX_G; ++i) my.y[i] = 0.0;
    int rc;
    if ((rc = mes_table(g, include_noise, y_std, "gp_mes_logsurv"))) return rc;
    launch_mes_logsurv(g->s, g->dMean, g->dVar, g->M, y_mean, y_std, my, g->mes.dPart);
    HIPCHK(hipMemcpyAsync(out, g->mes.dPart + mes_chunks(g->M) * MES_MAX_G, sizeof(double) * G, hipMemcpyDeviceToHost, g->s));
    GP_SYNC(g->s);
    return 0;
}

extern "C" int gp_mes_bracket(gp_t *g, int include_noise, double y_mean, double y_std, double nsig, double *lo, double *hi) {
    if (!g || !lo || !hi) return fail(GP_ERR_ARG, "null argument");
    GP_SCORING(g);
    if (!std::isfinite(y_mean)) return fail(GP_ERR_ARG, "gp_mes_bracket: y_mean must be finite");
    if (!(nsig >= 0.0) || !std::isfinite(nsig)) return fail(GP_ERR_ARG, "gp_mes_bracket: nsig must be finite and not negative");
    int rc;
    if ((rc = mes_table(g, include_noise, y_std, "gp_mes_bracket"))) return rc;
    launch_mes_bracket(g->s, g->dMean, g->dVar, g->M, y_mean, y_std, nsig, g->mes.dPart);
    double h[2] = {0.0, 0.0};
    HIPCHK(hipMemcpyAsync(h, g->mes.dPart + mes_chunks(g->M) * MES_MAX_G, sizeof(double) * 2, hipMemcpyDeviceToHost, g->s));
    GP_SYNC(g->s);
    *lo = h[0];
    *hi = h[1];
    return 0;
}
