// The knowledge gradient (include/gphip.h, gp_kg_*; kernels: csrc/kg.hip): the discretisation points of a fit and the scoring of
// candidate tables.  gp_kg_rows, the entry for a handful of locations by value, sits with the other rows entries (api_rows.hip).
#include "api_internal.h"

constexpr long KG_LD = GP_KG_MAX_A;   // leading dimension of a chunk's covariance block and rows of V_A: two tiles
static_assert(KG_LD % GP_TILE == 0, "V_A and C are padded tile operands");

// what every entry that touches the model's posterior asks of the context beyond a fit
static int check_kg_model(const gp_ctx *g) {
    GP_NO_LAPLACE(g, "the knowledge gradient");
    if (g->P != 1) return fail(GP_ERR_STATE, "the knowledge gradient needs P == 1");
    if (g->warp.n > 0) return fail(GP_ERR_STATE, "the knowledge gradient: an output warp is on");
    if (g->sp.fitted) return fail(GP_ERR_STATE, "the knowledge gradient: the context holds a sparse fit");
    if (g->ens.S > 0) return fail(GP_ERR_STATE, "the knowledge gradient: the context holds an ensemble");
    if (g->kp.gower) return fail(GP_ERR_STATE, "the knowledge gradient: not available for a Gower kernel");
    return 0;
}
static int check_y_std(double y_std) {
    return y_std > 0.0 && std::isfinite(y_std) ? 0 : fail(GP_ERR_ARG, "y_std must be positive and finite");
}

static void swap_buf(DevBuf<double> &a, DevBuf<double> &b) {
    std::swap(a.p, b.p);
    std::swap(a.cap, b.cap);
}

extern "C" int gp_kg_set_points(gp_t *g, const double *Xa, int A, double y_mean, double y_std, double *mu) {
    if (!g || !Xa) return fail(GP_ERR_ARG, "null argument");
    GP_FITTED(g);
    GP_NO_MEAN(g, "gp_kg_set_points");
    int rc;
    if ((rc = check_kg_model(g))) return rc;
    if (A < 1 || A > GP_KG_MAX_A) return fail(GP_ERR_ARG, "A out of range (1..%d)", GP_KG_MAX_A);
    for (long i = 0; i < (long)A * g->D; ++i)
        if (!std::isfinite(Xa[i])) return fail(GP_ERR_ARG, "gp_kg_set_points: a point is not finite");
    if (!std::isfinite(y_mean)) return fail(GP_ERR_ARG, "y_mean must be finite");
    if ((rc = check_y_std(y_std))) return rc;
    KgState &kg = g->kg;
    kg.A = 0;
    GP_SYNC(g->s);
    const long Npad = g->Npad;
    if ((rc = kg.dXa.reserve((long)GP_KG_MAX_A * GP_MAX_D))) return rc;
    if ((rc = kg.dVA.reserve(KG_LD * Npad))) return rc;
    if ((rc = kg.dMuA.reserve(GP_KG_MAX_A))) return rc;
    HIPCHK(hipMemcpy(kg.dXa, Xa, sizeof(double) * A * g->D, hipMemcpyHostToDevice));
    // the points take the candidates' place for one tile-path solve, as gp_es_set_representers runs it (S = K(Xa, X) L^-T in dT2,
    // zero padding rows); the table comes back afterwards, its cached posterior does not
    const long M0 = g->M;
    swap_buf(g->dXs, kg.dXa);
    g->M = A;
    const ChunkHook keep = [&](long m0, long mc, long mcpad) -> int {   // (one chunk unless option "mc_max" is below 256)
        HIPCHK(hipMemcpyAsync(kg.dVA + m0 * Npad, g->dT2, sizeof(double) * mcpad * Npad, hipMemcpyDeviceToDevice, g->s));
        return 0;
    };
    rc = ensure_out(g);
    if (!rc) rc = run_predict(g, 0, true, &keep);
    swap_buf(g->dXs, kg.dXa);
    g->M = M0;
    g->predicted = false;
    if (rc) return rc;
    std::vector<double> h(A);
    HIPCHK(hipMemcpyAsync(kg.dMuA, g->dMean, sizeof(double) * A, hipMemcpyDeviceToDevice, g->s));
    HIPCHK(hipMemcpyAsync(h.data(), g->dMean, sizeof(double) * A, hipMemcpyDeviceToHost, g->s));
    GP_SYNC(g->s);
    if (mu)
        for (int i = 0; i < A; ++i) mu[i] = h[i] * y_std + y_mean;
    kg.A = A;
    return 0;
}

extern "C" int gp_kg_info(gp_t *g, int *A) {
    if (!g || !A) return fail(GP_ERR_ARG, "null argument");
    *A = g->kg.A;
    return 0;
}

int kg_ready(gp_ctx *g, double y_std) {
    int rc;
    if ((rc = check_kg_model(g))) return rc;
    if (g->kg.A < 1) return fail(GP_ERR_STATE, "gp_kg_set_points first (a new fit drops the points)");
    return check_y_std(y_std);
}

// +KG of the resident candidates into dAcq (not drained)
static int run_kg_acq(gp_ctx *g, double y_std) {
    int rc;
    if ((rc = kg_ready(g, y_std))) return rc;
    KgState &kg = g->kg;
    if ((rc = ensure_out(g))) return rc;
    const long Npad = g->Npad;
    const long mc_max = std::min(g->mc_max, round_up(g->M, GP_TILE));   // the chunks of run_predict
    if ((rc = kg.dC.reserve(mc_max * KG_LD))) return rc;
    const int at = (int)(round_up(kg.A, GP_TILE) / GP_TILE);
    const ChunkHook score = [&](long m0, long mc, long mcpad) -> int {
        // C = K(Xs, Xa) - (K(Xs, X) L^-T) V_A^T for the chunk whose solved rows dT2 holds: the GEMM entropy search runs against V_R
        launch_cross_k(g->s, kg.dC, KG_LD, g->dXs + m0 * g->D, mc, mcpad, kg.dXa, kg.A, at * GP_TILE, g->kp);
        gemm(g, g->s, 1, kg.dC, KG_LD, g->dT2, Npad, kg.dVA, Npad, 1, (int)Npad, TileSet{0, (int)(mcpad / GP_TILE), 0, at, 0});
        launch_kg_score(g->s, kg.dC, KG_LD, g->dMean + m0, g->dVar + m0, mc, y_std, g->noise, kg.A, kg.dMuA, g->dAcq + m0);
        return 0;
    };
    // the variance WITHOUT noise (the lines' slopes take the latent variance); the tile path for every M: the solved rows are a
    // padded GEMM operand
    return run_predict(g, 0, true, &score);
}

extern "C" int gp_kg_acq(gp_t *g, double y_std, double *out) {
    if (!g || !out) return fail(GP_ERR_ARG, "null argument");
    GP_SCORING(g);
    GP_NO_MEAN(g, "gp_kg_acq");
    int rc;
    if ((rc = run_kg_acq(g, y_std))) return rc;
    return scores_out(g, g->dAcq, nullptr, g->M, g->D, out, nullptr);
}

// argbest and top-k run the candidate tables' shared selector over the score vector in dAcq, as gp_es_acq_argbest does
extern "C" int gp_kg_acq_argbest(gp_t *g, double y_std, int sense, int64_t *idx, double *val) {
    if (!g || !idx || !val) return fail(GP_ERR_ARG, "null argument");
    GP_SCORING(g);
    GP_NO_MEAN(g, "gp_kg_acq_argbest");
    int rc;
    if ((rc = check_sense(sense))) return rc;
    if ((rc = run_kg_acq(g, y_std))) return rc;
    return select_best(g, g->dAcq, g->M, sense, nullptr, 0, idx, val);
}

extern "C" int gp_kg_acq_topk(gp_t *g, double y_std, int sense, int k, int64_t *idx, double *val) {
    if (!g || !idx || !val) return fail(GP_ERR_ARG, "null argument");
    GP_SCORING(g);
    GP_NO_MEAN(g, "gp_kg_acq_topk");
    int rc;
    if ((rc = check_sense(sense))) return rc;
    if ((rc = check_k(k))) return rc;
    if ((rc = run_kg_acq(g, y_std))) return rc;
    return select_topk(g, g->dAcq, g->M, sense, k, idx, val);
}
