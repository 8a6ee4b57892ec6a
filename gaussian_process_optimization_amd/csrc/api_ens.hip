// The ensemble entry points: S hyper-parameter members over the context's (X, Y) with RESIDENT posteriors, and the acquisitions
// integrated over them -- GPModel_MCMC (GPyOpt/GPyOpt/models/gpmodel.py:180-355) with acquisitions/{EI,MPI,LCB}_mcmc.py.
// The reference writes each HMC sample into the model and refactorises for every acquisition call (gpmodel.py:266-272, 307-315)
// and again for get_fmin (:285-291): 2 S Cholesky factorisations per L-BFGS evaluation.  Here gp_ens_fit factors the S members
// once, in the lockstep launch sequences of gp_fit_grad_batch (struct Members), and KEEPS each member's alpha, inverse factor,
// parameters, jitter and fmin; a scoring call is then matrix-vector work over the S inverse factors in the launches of one
// model's call (ens_rows.hip), or, over the resident candidate table, one cross covariance per member, one batched GEMM against
// the inverse factors and one reduce.  Always true fp64.  The ensemble lives beside the context's own fit (EnsState).
#include "api_internal.h"

#define GP_ENS_MAX_NPAD 2048   // the batched fit's cap
#define GP_ENS_TABLE_CHUNK 512 // candidate rows per pass of the table route

static int ens_ready(gp_ctx *g) {
    GP_DEAD_CHECK(g);
    GP_NO_MEAN(g, "the ensemble entry points");
    if (g->ens.S < 1) return fail(GP_ERR_STATE, "gp_ens_fit first");
    HIPCHK(hipSetDevice(g->device));
    return 0;
}

static const double *ens_noise(const gp_ctx *g) { return g->ens.dTab; }
static const double *ens_fmin(const gp_ctx *g) { return g->ens.dTab + GP_ENS_MAX_S; }

extern "C" int gp_ens_fit(gp_t *g, int S, const double *variance, const double *lengthscale, const double *noise, int maxtries,
                          double *lml, double *logdet, double *jitter_used, double *fmin) {
    if (!g || !variance || !lengthscale || !noise) return fail(GP_ERR_ARG, "null argument");
    GP_DEAD_CHECK(g);
    GP_NO_MEAN(g, "gp_ens_fit");
    if (!g->have_data) return fail(GP_ERR_STATE, "gp_set_data before gp_ens_fit");
    // what the shapes alone decide comes first: a data set the ensemble cannot take is refused before any parameters are asked for
    if (S < 1 || S > GP_ENS_MAX_S) return fail(GP_ERR_ARG, "gp_ens_fit takes 1 <= S <= %d members (got %d)", GP_ENS_MAX_S, S);
    if (g->Npad > GP_ENS_MAX_NPAD)
        return fail(GP_ERR_ARG, "gp_ens_fit covers Npad <= %d (N = %ld pads to %ld)", GP_ENS_MAX_NPAD, g->N, g->Npad);
    if (g->P != 1) return fail(GP_ERR_ARG, "gp_ens_fit needs P == 1");
    if (!g->have_params) return fail(GP_ERR_STATE, "gp_set_params before gp_ens_fit");
    if (g->kp.gower)   // the lengthscale does not enter a Gower K: sampling it is sampling its prior
        return fail(GP_ERR_STATE, "gp_ens_fit: the Gower option is on (gp_set_gower)");
    if (g->warp.n > 0) return fail(GP_ERR_STATE, "gp_ens_fit: an output warp is on (gp_set_output_warp)");
    std::vector<KernParams> kp;
    if (int e = member_params(g, S, variance, lengthscale, noise, &kp)) return e;
    HIPCHK(hipSetDevice(g->device));
    EnsState &en = g->ens;
    en.S = 0;   // invalid until every member is factored and kept

    const long N = g->N, Npad = g->Npad;
    const int P = 1, nt = (int)(Npad / GP_TILE);
    int rc;
    if ((rc = en.dLi.reserve((long)S * Npad * Npad))) return rc;
    if ((rc = en.dAlpha.reserve((long)S * Npad))) return rc;
    if ((rc = en.dTab.reserve(2 * GP_ENS_MAX_S))) return rc;
    if ((rc = en.dKp.reserve((long)sizeof(KernParams) * GP_ENS_MAX_S))) return rc;
    std::vector<double> diag(S), diag0(S), jit(S, 0.0);
    for (int r = 0; r < S; ++r) ky_diag(kp[r], noise[r], &diag[r], &diag0[r]);
    // the batched fit's members (batch_members), used without Ky^-1 and the gradient passes; behind them the training mean of one
    Members m;
    double *dJit, *dMu;
    if ((rc = batch_members(g, kp, diag, Npad, 0, &m, &dJit, &dMu, nullptr))) return rc;
    m.X = g->dX;   // shared by the members: strides 0
    m.Y = g->dY;
    m.jit = jit.data();

    // the per-member jitter ladder; one member that cannot be factored fails the call: the ensemble stays invalid
    std::vector<int> st(S, 0);
    if ((rc = ky_ladder(g, m, maxtries, diag0, jit, dJit, st))) return rc;
    for (int r = 0; r < S; ++r)
        if ((rc = ladder_failure(st[r]))) return rc;

    panel_inv_members(g, m);
    alpha_lml(g, g->s, m);
    identity_blocks(g->s, m.T, Npad, S);
    solve_rows(g, m, nt, 1);   // L^-T into T2
    // kept: Li = (L^-T)^T with exact zeros above the diagonal, alpha, and the minimum of the training mean y - d alpha
    // (GPModel_MCMC.get_fmin, gpmodel.py:285-291), d the whole diagonal the member's K got
    for (int r = 0; r < S; ++r) {
        launch_transpose_tri(g->s, en.dLi + (long)r * Npad * Npad, m.T2 + (long)r * m.sT, Npad, 0);
        launch_train_mean_identity(g->s, g->dY, m.alpha + (long)r * m.sV, diag[r] + jit[r], N, dMu);
        launch_argbest(g->s, dMu, N, -1, en.dTab + GP_ENS_MAX_S + r, g->dRedI + RED_RESULT.off, g->dRedV + RED_PARTIAL.off,
                       g->dRedI + RED_PARTIAL.off);
    }
    HIPCHK(hipMemcpyAsync(en.dAlpha, m.alpha, sizeof(double) * S * Npad, hipMemcpyDeviceToDevice, g->s));
    HIPCHK(hipMemcpyAsync(en.dKp.p, kp.data(), sizeof(KernParams) * S, hipMemcpyHostToDevice, g->s));
    HIPCHK(hipMemcpyAsync(en.dTab, noise, sizeof(double) * S, hipMemcpyHostToDevice, g->s));
    if ((rc = en.pass.restart(g->s))) return rc;   // the arrival counters start again with every ensemble: another S leaves members that never counted
    std::vector<double> sc((size_t)m.sS * S);
    en.fmin.assign(S, 0.0);
    HIPCHK(hipMemcpyAsync(sc.data(), m.scal, sizeof(double) * m.sS * S, hipMemcpyDeviceToHost, g->s));
    HIPCHK(hipMemcpyAsync(en.fmin.data(), en.dTab + GP_ENS_MAX_S, sizeof(double) * S, hipMemcpyDeviceToHost, g->s));
    GP_SYNC(g->s);

    for (int r = 0; r < S; ++r) {
        const double *s = sc.data() + (size_t)m.sS * r;
        if (logdet) logdet[r] = s[SCAL_LOGDET.off];
        if (lml) lml[r] = lml_from_scalars(N, P, s);
        if (jitter_used) jitter_used[r] = jit[r];
        if (fmin) fmin[r] = en.fmin[r];
    }
    en.kp = kp;
    en.noise.assign(noise, noise + S);
    en.jitter = jit;
    en.S = S;
    return 0;
}

extern "C" int gp_ens_info(gp_t *g, int *S) {
    if (!g || !S) return fail(GP_ERR_ARG, "null argument");
    GP_DEAD_CHECK(g);
    *S = g->ens.S;
    return 0;
}

// ---- the rows route ------------------------------------------------------------------------------------------------------------
static int ens_rows_table(gp_ctx *g, EnsRows *t) {
    EnsState &en = g->ens;
    const long Npad = g->Npad, S = en.S;
    const int nt = (int)(Npad / GP_TILE);
    const long nch = (nt - 1) / 8 + 1, nrb = (long)nt * (GP_TILE / ENS_ROWS_RB);
    t->sW = nch * ROWS_MAX_M * Npad;
    t->sB = nrb * ROWS_MAX_M * Npad;
    t->sM = nch * ROWS_MAX_M;
    t->sV = nrb * ROWS_MAX_M;
    t->sG = (long)rows_gpart_elems(g->N);
    int rc;
    if ((rc = en.dWork.reserve(S * (t->sW + t->sB + t->sM + t->sV + t->sG + ENS_POST_STRIDE)))) return rc;
    t->wpart = en.dWork;
    t->bpart = t->wpart + S * t->sW;
    t->meanpart = t->bpart + S * t->sB;
    t->vpart = t->meanpart + S * t->sM;
    t->gpart = t->vpart + S * t->sV;
    t->post = t->gpart + S * t->sG;
    if ((rc = en.pass.ready(g->s))) return rc;
    t->counter = en.pass.counter;
    t->Li = en.dLi;
    t->sLi = Npad * Npad;
    t->alpha = en.dAlpha;
    t->sAlpha = Npad;
    t->kpt = (const KernParams *)en.dKp.p;
    t->noise = ens_noise(g);
    t->fmin = ens_fmin(g);
    return 0;
}

// passes of up to ROWS_MAX_M locations (four per pass is what the ensemble takes: no wide pass): every member's counter takes
// rows_finish_grid(N) arrivals, the ensemble's S.  post (when given) receives the S members' result blocks of each pass before
// unpack(m0, mc, block) runs
template <class Unpack>
static int ens_passes(gp_ctx *g, const double *Xs, int M, int want_grad, int include_noise, int acq_on, int type, double par,
                      std::vector<double> *post, Unpack unpack) {
    int rc;
    EnsRows t;
    if ((rc = ens_rows_table(g, &t))) return rc;
    EnsState &en = g->ens;
    if (post) post->resize((size_t)en.S * ENS_POST_STRIDE);
    // locations per pass: ROWS_MAX_M while their coordinates fit the kernel arguments (D <= 32), else what fits (3 at D = 33, 2 at
    // D = GP_MAX_D); a location's bits do not depend on its company, so the split is invisible in the results
    return rows_passes(g, en.pass, Xs, M, std::min(ROWS_MAX_M, ROWS_MAX_XS / g->D),
                       [&](const RowsX &rx, const PassReport &r, unsigned *arrivals) {
                           launch_ens_rows(g->s, t, en.S, rx, g->dX, g->N, g->Npad, want_grad, include_noise, acq_on, acq_base(type), par, r);
                           // the cost does not depend on the member: the quotient goes under the average, behind the pass
                           if (acq_on && acq_per_cost(type)) cost_divide_block(g, rx, want_grad != 0, r.out, rows_layout(rx.M));
                           if (post)
                               HIPCHK(hipMemcpyAsync(post->data(), t.post, sizeof(double) * en.S * ENS_POST_STRIDE, hipMemcpyDeviceToHost, g->s));
                           arrivals[0] = rows_finish_grid(g->N);
                           arrivals[1] = (unsigned)en.S;
                           return 0;
                       },
                       unpack);
}

extern "C" int gp_ens_predict_rows(gp_t *g, const double *Xs, int64_t M, int include_noise, double *mean, double *var, double *dmdx,
                                   double *dvdx) {
    if (!g || !Xs) return fail(GP_ERR_ARG, "null argument");
    int rc;
    if ((rc = ens_ready(g))) return rc;
    if (M < 1 || M > ROWS_WIDE_M) return fail(GP_ERR_ARG, "gp_ens_predict_rows takes 1 <= M <= %d locations", ROWS_WIDE_M);
    if ((dmdx == nullptr) != (dvdx == nullptr)) return fail(GP_ERR_ARG, "dmdx and dvdx come together");
    const int D = g->D, S = g->ens.S;
    std::vector<double> post;
    return ens_passes(g, Xs, (int)M, dmdx != nullptr, include_noise, 0, GP_ACQ_EI, 0.0, &post, [&](int m0, int mc, const double *) {
        const int MV = rows_layout(mc);
        for (int z = 0; z < S; ++z) {
            const double *o = post.data() + (size_t)z * ENS_POST_STRIDE;
            for (int mm = 0; mm < mc; ++mm) {
                const long at = (long)z * M + m0 + mm;
                if (mean) mean[at] = o[mm];
                if (var) var[at] = o[MV + mm];
                if (dmdx) {
                    memcpy(dmdx + at * D, o + 3 * MV + (long)mm * D, sizeof(double) * D);
                    memcpy(dvdx + at * D, o + 3 * MV + (long)MV * D + (long)mm * D, sizeof(double) * D);
                }
            }
        }
    });
}

static int ens_check_acq(const gp_ctx *g, int type) {
    if (acq_base(type) < GP_ACQ_EI || acq_base(type) > GP_ACQ_MPI) return fail(GP_ERR_ARG, "unknown acquisition %d", type);
    return check_per_cost(g, type, false);
}

extern "C" int gp_ens_acq_rows(gp_t *g, const double *Xs, int64_t M, int type, double par, double *out, double *dout) {
    if (!g || !Xs || !out) return fail(GP_ERR_ARG, "null argument");
    int rc;
    if ((rc = ens_ready(g))) return rc;
    if (M < 1 || M > ROWS_WIDE_M) return fail(GP_ERR_ARG, "gp_ens_acq_rows takes 1 <= M <= %d locations", ROWS_WIDE_M);
    if ((rc = ens_check_acq(g, type))) return rc;
    const int D = g->D;
    return ens_passes(g, Xs, (int)M, dout != nullptr, 1, 1, type, par, nullptr, [&](int m0, int mc, const double *o) {   // with_noise, gpmodel.py:271
        const int MV = rows_layout(mc);
        for (int mm = 0; mm < mc; ++mm) {
            out[m0 + mm] = o[2 * MV + mm];
            if (dout) memcpy(dout + (long)(m0 + mm) * D, o + 3 * MV + 2L * MV * D + (long)mm * D, sizeof(double) * D);
        }
    });
}

// ---- the table route -------------------------------------------------------------------------------------------------------------
// scores of the resident candidates (gp_set_candidates) into en.dAcq
static int ens_table_scores(gp_ctx *g, int type, double par) {
    EnsState &en = g->ens;
    if (g->M < 1) return fail(GP_ERR_STATE, "gp_set_candidates first");
    int rc;
    if ((rc = ens_check_acq(g, type))) return rc;
    const long M = g->M, N = g->N, Npad = g->Npad, S = en.S;
    const int nt = (int)(Npad / GP_TILE);
    const long chunk = std::min<long>(GP_ENS_TABLE_CHUNK, round_up(M, GP_TILE));
    if ((rc = en.dKx.reserve(S * chunk * Npad))) return rc;
    if ((rc = en.dW.reserve(S * chunk * Npad))) return rc;
    if ((rc = en.dAcq.reserve(M))) return rc;
    for (long m0 = 0; m0 < M; m0 += chunk) {
        const long mc = std::min(chunk, M - m0), mcpad = round_up(mc, GP_TILE);
        for (int z = 0; z < S; ++z)
            launch_cross_k(g->s, en.dKx + z * chunk * Npad, Npad, g->dXs + m0 * g->D, mc, mcpad, g->dX, N, Npad, en.kp[z]);
        GemmOpt o;   // W_z = Kx_z Li_z^T for every member in one launch
        o.batch = o.members = (int)S;
        o.sC = o.sA = chunk * Npad;
        o.sB = Npad * Npad;
        gemm(g, g->s, 0, en.dW, Npad, en.dKx, Npad, en.dLi, Npad, 1, (int)Npad, TileSet{0, (int)(mcpad / GP_TILE), 0, nt, 0}, o);
        launch_ens_table_reduce(g->s, en.dKx, en.dW, chunk, Npad, N, en.dAlpha, Npad, (const KernParams *)en.dKp.p, ens_noise(g),
                                ens_fmin(g), (int)S, acq_base(type), par, mc, en.dAcq + m0);
    }
    if (acq_per_cost(type)) return cost_divide(g, g->dXs, M, false, en.dAcq, nullptr);   // after the average over the members
    return 0;
}

extern "C" int gp_ens_acq(gp_t *g, int type, double par, double *out) {
    if (!g || !out) return fail(GP_ERR_ARG, "null argument");
    int rc;
    if ((rc = ens_ready(g))) return rc;
    if ((rc = ens_table_scores(g, type, par))) return rc;
    return scores_out(g, g->ens.dAcq, nullptr, g->M, g->D, out, nullptr);
}

extern "C" int gp_ens_acq_argbest(gp_t *g, int type, double par, int sense, int64_t *idx, double *val) {
    if (!g || !idx || !val) return fail(GP_ERR_ARG, "null argument");
    int rc;
    if ((rc = ens_ready(g))) return rc;
    if ((rc = check_sense(sense))) return rc;
    if ((rc = ens_table_scores(g, type, par))) return rc;
    return select_best(g, g->ens.dAcq, g->M, sense, nullptr, 0, idx, val);
}
