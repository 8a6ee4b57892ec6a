// Entropy search: the representers' posterior, the EP sweeps of p_min, the belief and the scoring of candidate tables.
// Reference: GPyOpt/GPyOpt/acquisitions/ES.py, util/epmgp.py.  Kernels: es.hip.
#include "api_internal.h"

// layout of EsState::dBelief (doubles)
constexpr long ESB_LOGP = 0, ESB_U = GP_ES_MAX_R, ESB_GT = 2 * GP_ES_MAX_R, ESB_W = ESB_GT + GP_ES_MAX_R * GP_ES_MAX_R,
               ESB_QT = ESB_W + GP_ES_MAX_S;

static int check_R(int R) { return R >= 1 && R <= GP_ES_MAX_R ? 0 : fail(GP_ERR_ARG, "R out of range (1..%d)", GP_ES_MAX_R); }
// what every entry that touches the model's posterior asks of the context beyond a fit
static int check_es_model(const gp_ctx *g) {
    GP_NO_LAPLACE(g, "entropy search");
    if (g->P != 1) return fail(GP_ERR_ARG, "entropy search needs P == 1");
    if (g->warp.n > 0) return fail(GP_ERR_STATE, "entropy search: an output warp is on");
    if (g->sp.fitted) return fail(GP_ERR_STATE, "entropy search: the context holds a sparse fit");
    if (g->ens.S > 0) return fail(GP_ERR_STATE, "entropy search: the context holds an ensemble");
    return 0;
}

static void swap_buf(DevBuf<double> &a, DevBuf<double> &b) {
    std::swap(a.p, b.p);
    std::swap(a.cap, b.cap);
}

extern "C" int gp_es_set_representers(gp_t *g, const double *Xr, int R, double y_mean, double y_std, double *mu, double *cov) {
    if (!g || !Xr || !mu || !cov) return fail(GP_ERR_ARG, "null argument");
    GP_FITTED(g);
    GP_NO_MEAN(g, "gp_es_set_representers");
    int rc;
    if ((rc = check_R(R))) return rc;
    if ((rc = check_es_model(g))) return rc;
    EsState &es = g->es;
    es.R = 0;
    es.belief = false;
    GP_SYNC(g->s);
    const long Npad = g->Npad;
    if ((rc = es.dXr.reserve((long)GP_ES_MAX_R * GP_MAX_D))) return rc;
    if ((rc = es.dVR.reserve(GP_TILE * Npad))) return rc;
    if ((rc = g->dCov.reserve((long)GP_TILE * GP_TILE))) return rc;
    HIPCHK(hipMemcpy(es.dXr, Xr, sizeof(double) * R * g->D, hipMemcpyHostToDevice));
    // the representers take the candidates' place for one tile-path solve, as gp_predict_full_cov runs it (S = K(Xr, X) L^-T in
    // dT2, one chunk with zero padding rows); the table comes back afterwards, its cached posterior does not
    const long M0 = g->M;
    swap_buf(g->dXs, es.dXr);
    g->M = R;
    rc = ensure_out(g);
    if (!rc) rc = run_predict(g, 1, true);
    if (!rc) {
        launch_kbuild(g->s, g->dCov, GP_TILE, g->dXs, R, GP_TILE, g->kp, 0.0, 1);   // K(Xr, Xr)
        gemm(g, g->s, 1, g->dCov, GP_TILE, g->dT2, Npad, g->dT2, Npad, 1, (int)Npad, TileSet{0, 1, 0, 1, 0});
        launch_add_diag(g->s, g->dCov, GP_TILE, R, g->noise);
    }
    swap_buf(g->dXs, es.dXr);
    g->M = M0;
    g->predicted = false;
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(es.dVR, g->dT2, sizeof(double) * GP_TILE * Npad, hipMemcpyDeviceToDevice, g->s));
    HIPCHK(hipMemcpyAsync(mu, g->dMean, sizeof(double) * R, hipMemcpyDeviceToHost, g->s));
    GP_SYNC(g->s);
    HIPCHK(hipMemcpy2D(cov, sizeof(double) * R, g->dCov, sizeof(double) * GP_TILE, sizeof(double) * R, R, hipMemcpyDeviceToHost));
    for (int i = 0; i < R; ++i) mu[i] = mu[i] * y_std + y_mean;
    for (long e = 0; e < (long)R * R; ++e) cov[e] *= y_std * y_std;
    es.R = R;
    return 0;
}

extern "C" int gp_es_pmin(gp_t *g, const double *mu, const double *cov, int R, int max_sweeps, double tol, double *P, double *MP,
                          double *logS, int *status, int *sweeps) {
    if (!g || !mu || !cov || !status || !sweeps) return fail(GP_ERR_ARG, "null argument");
    GP_DEAD_CHECK(g);
    GP_NO_MEAN(g, "gp_es_pmin");
    int rc;
    if ((rc = check_R(R))) return rc;
    if (max_sweeps < 1 || max_sweeps > 100000) return fail(GP_ERR_ARG, "max_sweeps out of range (1..100000)");
    if (R == 1) {   // no factor to visit: the first sweep's sum |d| is 0
        status[0] = 0;
        sweeps[0] = 1;
        return 0;
    }
    if (!P || !MP || !logS) return fail(GP_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(g->device));
    const long nR = R, nS = nR * (R - 1);
    // dEp: mu [R], cov [R, R], P, MP, logS [R, R - 1] each, then status [R] and sweeps [R] as ints
    if ((rc = g->es.dEp.reserve(nR + nR * nR + 3 * nS + nR))) return rc;
    double *dmu = g->es.dEp, *dcov = dmu + nR, *dP = dcov + nR * nR, *dMP = dP + nS, *dLS = dMP + nS;
    int *dst = (int *)(dLS + nS), *dsw = dst + R;
    HIPCHK(hipMemcpyAsync(dmu, mu, sizeof(double) * nR, hipMemcpyHostToDevice, g->s));
    HIPCHK(hipMemcpyAsync(dcov, cov, sizeof(double) * nR * nR, hipMemcpyHostToDevice, g->s));
    launch_es_pmin(g->s, dmu, dcov, R, max_sweeps, tol, dP, dMP, dLS, dst, dsw);
    HIPCHK(hipMemcpyAsync(P, dP, sizeof(double) * nS, hipMemcpyDeviceToHost, g->s));
    HIPCHK(hipMemcpyAsync(MP, dMP, sizeof(double) * nS, hipMemcpyDeviceToHost, g->s));
    HIPCHK(hipMemcpyAsync(logS, dLS, sizeof(double) * nS, hipMemcpyDeviceToHost, g->s));
    HIPCHK(hipMemcpyAsync(status, dst, sizeof(int) * R, hipMemcpyDeviceToHost, g->s));
    HIPCHK(hipMemcpyAsync(sweeps, dsw, sizeof(int) * R, hipMemcpyDeviceToHost, g->s));
    GP_SYNC(g->s);
    return 0;
}

extern "C" int gp_es_set_belief(gp_t *g, const double *logP, const double *u, const double *G, const double *Q, int R,
                                const double *W, int S) {
    if (!g || !logP || !u || !G || !Q || !W) return fail(GP_ERR_ARG, "null argument");
    GP_FITTED(g);
    GP_NO_MEAN(g, "gp_es_set_belief");
    int rc;
    if ((rc = check_R(R))) return rc;
    if (S < 1 || S > GP_ES_MAX_S) return fail(GP_ERR_ARG, "S out of range (1..%d)", GP_ES_MAX_S);
    EsState &es = g->es;
    if (es.R < 1) return fail(GP_ERR_STATE, "gp_es_set_representers first");
    if (R != es.R) return fail(GP_ERR_STATE, "the belief has %d entries, the resident representers are %d", R, es.R);
    es.belief = false;
    const long n = R, n3 = n * n * n;
    if ((rc = es.dBelief.reserve(ESB_QT + (long)GP_ES_MAX_R * GP_ES_MAX_R * GP_ES_MAX_R))) return rc;
    // the belief index goes last: lane i of the scoring kernel reads Qt[a, b, i], Gt[a, i]
    std::vector<double> h(ESB_QT + n3, 0.0);
    for (long i = 0; i < n; ++i) {
        h[ESB_LOGP + i] = logP[i];
        h[ESB_U + i] = u[i];
        for (long a = 0; a < n; ++a) {
            h[ESB_GT + a * n + i] = G[i * n + a];
            for (long b = 0; b < n; ++b) h[ESB_QT + (a * n + b) * n + i] = Q[(i * n + a) * n + b];
        }
    }
    for (int w = 0; w < S; ++w) h[ESB_W + w] = W[w];
    GP_SYNC(g->s);
    HIPCHK(hipMemcpy(es.dBelief, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice));
    es.S = S;
    es.belief = true;
    return 0;
}

int es_ready(gp_ctx *g, double y_std) {
    int rc;
    if ((rc = check_es_model(g))) return rc;
    if (g->es.R < 1) return fail(GP_ERR_STATE, "gp_es_set_representers first (a new fit drops the representers)");
    if (!g->es.belief) return fail(GP_ERR_STATE, "gp_es_set_belief first");
    if (!(y_std > 0.0) || !std::isfinite(y_std)) return fail(GP_ERR_ARG, "y_std must be positive and finite");
    return 0;
}
EsBelief es_belief(const gp_ctx *g) {
    const double *b = g->es.dBelief;
    return EsBelief{b + ESB_QT, b + ESB_GT, b + ESB_LOGP, b + ESB_U, b + ESB_W};
}

// the scores of the resident candidates into dAcq (not drained)
static int run_es_acq(gp_ctx *g, double y_std) {
    int rc;
    if ((rc = es_ready(g, y_std))) return rc;
    EsState &es = g->es;
    if ((rc = ensure_out(g))) return rc;
    const long Npad = g->Npad;
    const long mc_max = std::min(g->mc_max, round_up(g->M, GP_TILE));   // the chunks of run_predict
    if ((rc = es.dC.reserve(mc_max * GP_TILE))) return rc;
    const EsBelief b = es_belief(g);
    const ChunkHook score = [&](long m0, long mc, long mcpad) -> int {
        // C = K(Xs, Xr) - (K(Xs, X) L^-T) V_R^T for the chunk whose solved rows dT2 holds
        launch_cross_k(g->s, es.dC, GP_TILE, g->dXs + m0 * g->D, mc, mcpad, es.dXr, es.R, GP_TILE, g->kp);
        gemm(g, g->s, 1, es.dC, GP_TILE, g->dT2, Npad, es.dVR, Npad, 1, (int)Npad, TileSet{0, (int)(mcpad / GP_TILE), 0, 1, 0});
        launch_es_score(g->s, es.dC, GP_TILE, g->dVar + m0, mc, y_std, es.R, b.Qt, b.Gt, b.logP, b.u, b.W, es.S,
                        g->dAcq + m0);
        return 0;
    };
    // the variance WITHOUT noise (ES.py:199); the tile path for every M: the solved rows are a padded GEMM operand
    return run_predict(g, 0, true, &score);
}

extern "C" int gp_es_acq(gp_t *g, double y_std, double *out) {
    if (!g || !out) return fail(GP_ERR_ARG, "null argument");
    GP_SCORING(g);
    GP_NO_MEAN(g, "gp_es_acq");
    int rc;
    if ((rc = run_es_acq(g, y_std))) return rc;
    return scores_out(g, g->dAcq, nullptr, g->M, g->D, out, nullptr);
}

extern "C" int gp_es_acq_argbest(gp_t *g, double y_std, int sense, int64_t *idx, double *val) {
    if (!g || !idx || !val) return fail(GP_ERR_ARG, "null argument");
    GP_SCORING(g);
    GP_NO_MEAN(g, "gp_es_acq_argbest");
    int rc;
    if ((rc = check_sense(sense))) return rc;
    if ((rc = run_es_acq(g, y_std))) return rc;
    return select_best(g, g->dAcq, g->M, sense, nullptr, 0, idx, val);
}
