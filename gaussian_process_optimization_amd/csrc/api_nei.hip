// Noisy expected improvement (include/gphip.h, gp_nei_*; kernels: csrc/nei.hip): the fantasies of a (model, twin) pair and the
// scoring of the twin's candidate table.  gp_nei_rows, the entry for a handful of locations by value, sits with the other rows
// entries (api_rows.hip).  The state lives on the twin (NeiState, api_internal.h); the model is only read while gp_nei_set runs.
#include "api_internal.h"

static_assert(GP_NEI_MAX_S == NEI_SPAD && NEI_SPAD <= PATHS_MAX_SPAD && NEI_SPAD <= GP_MAX_RHS, "the fantasies ride as right-hand-side rows of one tile");
static_assert(NEI_SPAD % PATHS_MMA == 0, "whole tiles of the table's product");

// what NEI asks of either handle beyond a fit (before anything is launched or changed)
static int check_nei_handle(const gp_ctx *g, const char *which) {
    if (!g->fitted) return fail(GP_ERR_STATE, "noisy EI: the %s is not fitted (gp_fit first)", which);
    if (g->lap.on) return fail(GP_ERR_STATE, "noisy EI: the %s is a Laplace-fitted handle", which);
    if (g->P != 1) return fail(GP_ERR_STATE, "noisy EI: the %s needs P == 1", which);
    if (g->kp.gower) return fail(GP_ERR_STATE, "noisy EI: the %s has a Gower kernel", which);
    if (g->mean.on()) return fail(GP_ERR_STATE, "noisy EI: the %s has a mean function", which);
    if (g->warp.n > 0) return fail(GP_ERR_STATE, "noisy EI: the %s has an output warp", which);
    if (g->sp.fitted) return fail(GP_ERR_STATE, "noisy EI: the %s holds a sparse fit", which);
    if (g->ens.S > 0) return fail(GP_ERR_STATE, "noisy EI: the %s holds an ensemble", which);
    return 0;
}

static int nei_model_unchanged(const gp_ctx *g, const char *who) {
    const NeiState &ne = g->nei;
    if (!ctx_fit_is(ne.model, ne.model_gen))
        return fail(GP_ERR_STATE, "%s: the model was refitted, changed or destroyed since gp_nei_set", who);
    return 0;
}

int nei_ready(gp_ctx *g, double y_mean, double y_std, const char *who) {
    int rc;
    if (g->nei.S < 1) return fail(GP_ERR_STATE, "%s: gp_nei_set first (a new fit of the twin drops the fantasies)", who);
    if ((rc = check_nei_handle(g, "twin"))) return rc;
    if ((rc = nei_model_unchanged(g, who))) return rc;
    if (!std::isfinite(y_mean)) return fail(GP_ERR_ARG, "%s: y_mean must be finite", who);
    if (!(y_std > 0.0) || !std::isfinite(y_std)) return fail(GP_ERR_ARG, "%s: y_std must be positive and finite", who);
    return 0;
}

extern "C" int gp_nei_set(gp_t *g, gp_t *model, int S, const double *Z, const double *E) {
    if (!g) return fail(GP_ERR_ARG, "null twin");
    GP_DEAD_CHECK(g);
    if (S < 0 || S > GP_NEI_MAX_S) return fail(GP_ERR_ARG, "gp_nei_set: S out of range (0..%d)", GP_NEI_MAX_S);
    if (S == 0) {   // clear
        g->nei.S = 0;
        g->nei.model = nullptr;
        return 0;
    }
    if (!model || !Z || !E) return fail(GP_ERR_ARG, "null argument");
    if (model == g) return fail(GP_ERR_ARG, "gp_nei_set: the twin and the model are one handle");
    if (!ctx_alive(model)) return fail(GP_ERR_ARG, "gp_nei_set: the model is not a live handle");
    GP_DEAD_CHECK(model);
    int rc;
    if ((rc = check_nei_handle(g, "twin"))) return rc;
    if ((rc = check_nei_handle(model, "model"))) return rc;
    if (g->device != model->device) return fail(GP_ERR_ARG, "gp_nei_set: the twin is on device %d, the model on %d", g->device, model->device);
    if (g->N != model->N || g->D != model->D)
        return fail(GP_ERR_ARG, "gp_nei_set: the twin holds N = %ld, D = %d, the model N = %ld, D = %d", g->N, g->D, model->N, model->D);
    const long N = g->N, Npad = g->Npad;
    const int D = g->D;
    if (g->kp.kernel != model->kp.kernel || g->ard != model->ard || memcmp(&g->kp.variance, &model->kp.variance, sizeof(double)) ||
        memcmp(g->kp.ls, model->kp.ls, sizeof(double) * D))
        return fail(GP_ERR_ARG, "gp_nei_set: kernel, ARD flag, variance and lengthscales of the two handles must be bit-equal");
    const double d = model->noise + 1e-8 + model->jitter, d0 = g->noise + 1e-8 + g->jitter;   // the factors' diagonals (ky_diag + the ladder's jitter)
    if (!(d > d0)) return fail(GP_ERR_ARG, "gp_nei_set: the model's diagonal %.3e must exceed the twin's %.3e (noisy EI is for noisy models)", d, d0);
    for (size_t i = 0; i < (size_t)S * N; ++i)
        if (!std::isfinite(Z[i]) || !std::isfinite(E[i])) return fail(GP_ERR_ARG, "gp_nei_set: a draw is not finite");
    HIPCHK(hipSetDevice(g->device));
    NeiState &ne = g->nei;
    GP_SYNC(g->s);          // nothing on either stream still reads what is about to go
    GP_SYNC(model->s);
    if ((rc = ne.dFlag.reserve(1))) return rc;
    HIPCHK(hipMemsetAsync(ne.dFlag, 0, sizeof(int), g->s));
    launch_nei_same_x(g->s, g->dX, model->dX, N * D, ne.dFlag);
    int differ = 0;
    HIPCHK(hipMemcpyAsync(&differ, ne.dFlag, sizeof(int), hipMemcpyDeviceToHost, g->s));
    GP_SYNC(g->s);
    if (differ) return fail(GP_ERR_ARG, "gp_nei_set: the two handles hold different X");
    ne.S = 0;
    ne.model = nullptr;
    if ((rc = ensure_panel_inv(g))) return rc;
    if ((rc = ensure_panel_inv(model))) return rc;
    if ((rc = ne.dA0.reserve((long)NEI_SPAD * Npad))) return rc;
    if ((rc = ne.dU.reserve((long)GP_TILE * Npad))) return rc;
    if ((rc = ne.dF.reserve((long)NEI_SPAD * Npad))) return rc;
    if ((rc = ne.dFstar.reserve(NEI_SPAD))) return rc;
    if ((rc = ne.dZt.reserve(2L * NEI_SPAD * Npad))) return rc;
    if ((rc = ne.dR.reserve((long)GP_TILE * Npad))) return rc;
    if ((rc = ne.dG.reserve((long)GP_TILE * Npad))) return rc;
    // Z transposed ([N, NEI_SPAD], zero columns beyond S: a lane per fantasy reads its row coalesced), E fantasy-major [S, Npad]
    std::vector<double> zt((size_t)N * NEI_SPAD, 0.0);
    for (int s = 0; s < S; ++s)
        for (long i = 0; i < N; ++i) zt[(size_t)i * NEI_SPAD + s] = Z[(size_t)s * N + i];
    double *dZt = ne.dZt, *dEm = ne.dZt + (long)NEI_SPAD * Npad;
    hipStream_t s = g->s;
    const size_t blk = sizeof(double) * (size_t)GP_TILE * Npad, blkS = sizeof(double) * (size_t)NEI_SPAD * Npad;
    HIPCHK(hipMemcpyAsync(dZt, zt.data(), sizeof(double) * zt.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(dEm, 0, blkS, s));
    HIPCHK(hipMemcpy2DAsync(dEm, sizeof(double) * Npad, E, sizeof(double) * N, sizeof(double) * N, S, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(ne.dR, 0, blk, s));
    HIPCHK(hipMemsetAsync(ne.dF, 0, blkS, s));
    HIPCHK(hipMemsetAsync(ne.dA0, 0, blkS, s));
    const double dd = d - d0, sd = std::sqrt(dd);
    // g = L0 Z^T into dR, then b = y - sd e into dF and the residual b - g in dR
    launch_nei_lz(s, g->dA, Npad, N, dZt, ne.dR, Npad);
    launch_nei_assemble(s, 0, S, N, model->dY, dEm, sd, dd, ne.dR, nullptr, ne.dF, Npad);
    GP_SYNC(s);   // (the host copy of Z goes out of scope below; the model's stream takes over)
    // V = Ky^-1 r against the MODEL's factor: the forward substitution as the candidate solve of one row tile (dR consumed,
    // dG = r L^-T), the backward one as alpha's (dR its workspace), into dA0 for now
    {
        Members m = ctx_members(model);
        m.T = ne.dR;
        m.T2 = ne.dG;
        solve_rows(model, m, 1, 0);
        launch_trsv_backward(model->s, model->dA, Npad, model->dInvP, model->invp_W, Npad, ne.dG, Npad, S, ne.dA0, ne.dR);
        GP_SYNC(model->s);
    }
    // F = b - dd V; its minima; a = K0^-1 F against the twin's factor, the forward substitution's result kept in dU
    launch_nei_assemble(s, 1, S, N, nullptr, nullptr, sd, dd, nullptr, ne.dA0, ne.dF, Npad);
    launch_nei_colmin(s, ne.dF, Npad, N, S, ne.dFstar);
    HIPCHK(hipMemsetAsync(ne.dR, 0, blk, s));
    HIPCHK(hipMemcpyAsync(ne.dR, ne.dF, blkS, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemsetAsync(ne.dA0, 0, blkS, s));
    {
        Members m = ctx_members(g);
        m.T = ne.dR;
        m.T2 = ne.dU;
        solve_rows(g, m, 1, 0);
        launch_trsv_backward(s, g->dA, Npad, g->dInvP, g->invp_W, Npad, ne.dU, Npad, S, ne.dA0, ne.dR);
    }
    GP_SYNC(s);
    ne.S = S;
    ne.d = d;
    ne.d0 = d0;
    ne.model = model;
    ne.model_gen = model->fit_gen;
    return 0;
}

extern "C" int gp_nei_info(gp_t *g, int *S, double *d_model, double *d_twin) {
    if (!g) return fail(GP_ERR_ARG, "null argument");
    GP_DEAD_CHECK(g);
    if (g->nei.S > 0) {
        int rc;
        if ((rc = nei_model_unchanged(g, "gp_nei_info"))) return rc;
    }
    if (S) *S = g->nei.S;
    if (d_model) *d_model = g->nei.S ? g->nei.d : 0.0;
    if (d_twin) *d_twin = g->nei.S ? g->nei.d0 : 0.0;
    return 0;
}

extern "C" int gp_nei_stats(gp_t *g, int64_t *linv_builds, int *pass_launches, int *pass_reads) {
    if (!g) return fail(GP_ERR_ARG, "null argument");
    GP_DEAD_CHECK(g);
    if (linv_builds) *linv_builds = g->linv_builds;
    if (pass_launches) *pass_launches = g->nei.pass_launches;
    if (pass_reads) *pass_reads = g->nei.pass_reads;
    return 0;
}

extern "C" int gp_nei_get(gp_t *g, double *F, double *fstar) {
    if (!g) return fail(GP_ERR_ARG, "null argument");
    GP_FITTED(g);
    int rc;
    if ((rc = nei_ready(g, 0.0, 1.0, "gp_nei_get"))) return rc;
    const NeiState &ne = g->nei;
    if (F)
        HIPCHK(hipMemcpy2DAsync(F, sizeof(double) * g->N, ne.dF, sizeof(double) * g->Npad, sizeof(double) * g->N, ne.S, hipMemcpyDeviceToHost, g->s));
    if (fstar) HIPCHK(hipMemcpyAsync(fstar, ne.dFstar, sizeof(double) * ne.S, hipMemcpyDeviceToHost, g->s));
    GP_SYNC(g->s);
    return 0;
}

// +NEI of the resident candidates into dAcq (not drained)
int nei_table_scores(gp_ctx *g, double par, double y_mean, double y_std, const char *who) {
    int rc;
    if ((rc = nei_ready(g, y_mean, y_std, who))) return rc;
    if (!std::isfinite(par)) return fail(GP_ERR_ARG, "%s: par must be finite", who);
    NeiState &ne = g->nei;
    const int Spad = (int)round_up(ne.S, PATHS_MMA);
    // the product's LDS is joint in D and S, as gp_paths_table documents
    if ((long)paths_table_lds_bytes(g->D, Spad) > g->lds_per_wg)
        return fail(GP_ERR_ARG, "%s: D = %d with %d fantasies needs %ld bytes of LDS per workgroup, the device gives %ld", who, g->D, ne.S,
                    (long)paths_table_lds_bytes(g->D, Spad), g->lds_per_wg);
    if ((rc = ensure_out(g))) return rc;
    if (!g->predicted || g->predicted_noise != 1)
        if ((rc = run_predict(g, 1))) return rc;   // the variance with the twin's noise, as gp_acq takes it
    if ((rc = ne.dTab.reserve((long)ne.S * g->M))) return rc;
    const long np = (long)paths_table_part_elems(g->M, g->N, ne.S);
    if (np && (rc = ne.dPart.reserve(np))) return rc;
    // gp_paths_table's kernel with A0 in V's place and NO feature term (F = 0: its loop has no trip), normaliser (0, 1): the
    // normalised means m_s(x_i) = sum_n k(x_i, X_n) A0[s, n] exactly as the accumulator leaves them
    const PathsPrior none{0, 0, Spad, 0.0, nullptr, nullptr, nullptr};
    launch_paths_table(g->s, none, ne.S, g->kp, g->dXs, g->M, g->dX, g->N, ne.dA0, g->Npad, 0.0, 1.0, ne.dTab, np ? ne.dPart.p : nullptr);
    launch_nei_score(g->s, ne.dTab, g->dVar, g->M, ne.S, ne.dFstar, par, y_mean, y_std, g->dAcq);
    return 0;
}

extern "C" int gp_nei_table(gp_t *g, double par, double y_mean, double y_std, double *out) {
    if (!g || !out) return fail(GP_ERR_ARG, "null argument");
    GP_SCORING(g);
    int rc;
    if ((rc = nei_table_scores(g, par, y_mean, y_std, "gp_nei_table"))) return rc;
    return scores_out(g, g->dAcq, nullptr, g->M, g->D, out, nullptr);
}

// argbest and top-k run the candidate tables' shared selector over the score vector in dAcq, as gp_kg_acq_argbest does
extern "C" int gp_nei_argbest(gp_t *g, double par, double y_mean, double y_std, int sense, int64_t *idx, double *val) {
    if (!g || !idx || !val) return fail(GP_ERR_ARG, "null argument");
    GP_SCORING(g);
    int rc;
    if ((rc = check_sense(sense))) return rc;
    if ((rc = nei_table_scores(g, par, y_mean, y_std, "gp_nei_argbest"))) return rc;
    return select_best(g, g->dAcq, g->M, sense, nullptr, 0, idx, val);
}

extern "C" int gp_nei_topk(gp_t *g, double par, double y_mean, double y_std, int sense, int k, int64_t *idx, double *val) {
    if (!g || !idx || !val) return fail(GP_ERR_ARG, "null argument");
    GP_SCORING(g);
    int rc;
    if ((rc = check_sense(sense))) return rc;
    if ((rc = check_k(k))) return rc;
    if ((rc = nei_table_scores(g, par, y_mean, y_std, "gp_nei_topk"))) return rc;
    return select_topk(g, g->dAcq, g->M, sense, k, idx, val);
}
