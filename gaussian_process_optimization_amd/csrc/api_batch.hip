// gp_fit_grad_batch: the LML and its hyper-parameter gradients for R parameter vectors over the context's (X, Y) in one call --
// the L-BFGS evaluations of R hyper-parameter restarts run in lockstep (GPRegression.optimize_restarts(parallel=True)).
// Reference: optimize_restarts over GPModel.updateModel (GPyOpt/GPyOpt/models/gpmodel.py:78-93), each evaluation being
// Model.objective_function + objective_function_gradients (GPy/GPy/core/model.py:96-127) of ExactGaussianInference
// (exact_gaussian_inference.py:37-74) with jitchol's ladder (linalg.py:56-81).
//
// The R vectors are R members (struct Members, api_internal.h) of the launch sequences gp_fit_grad's single-stream route is made
// of -- build_ky, factor_buf (128-column steps), the inverted diagonal panels, alpha_lml, solve_rows for L^-T, lauum, the gradient
// passes: the SAME host code, called here with nb = R and strides over g->dBatch where the context's own fit passes one member
// over its buffers.  The member is a batch index of every launch (blockIdx.z, or the GEMM's blockIdx.y), so R members cost the
// launches of ONE evaluation.  A launch over several members runs the body of its single-member kernel, and gemm() takes the
// instance the single call picks for one member's tiles: a member does the single call's arithmetic, bit for bit.
// The two warped models ride the same routine (fit_grad_members): gp_fit_grad_x_batch gives every member inputs of its own (the
// caller's warped X, Members::X at a stride) and adds the input-gradient pass with the member in blockIdx.z (gradx.hip);
// gp_fit_grad_warp_batch gives every member targets of its own (the raw targets through the member's tanh warp, Members::Y at a
// stride) and adds the warp's gradient sums, one workgroup per member (warp.hip).
// Left here: the checks, the per-member results, and the front end every batched entry shares -- the per-member parameters
// (member_params) and the carving of the batch's buffers (batch_members), which the ensemble (api_ens.hip) uses too; which
// members are factored again in which round of the jitter ladder is members_ladder's (api_factor.hip).  The batch has buffers
// of its own: the context's resident fit (L, alpha, Ky^-1, parameters, fitted / predicted state) is left as it was.  Always true
// fp64 (option "emulate_fp64" does not apply).
#include "api_internal.h"

#define GP_BATCH_MAX_R 64
#define GP_BATCH_MAX_NPAD 2048

// what the two warped batches add to the plain one (either may be null)
struct BatchInputs {          // gp_fit_grad_x_batch
    const double *Xw;         // host [R, N, D]: member r's (already warped) inputs
    double *dL_dX;            // host [R, N, D]
};
struct BatchWarp {            // gp_fit_grad_warp_batch
    int n_terms;
    const double *psi, *d;    // host [R, n_terms, 3] and [R]
    double *log_jacobian, *dpsi, *dd;   // host [R], [R, n_terms, 3], [R]
};
#define GP_BATCH_WARP_OUT (1 + GP_WARP_NPSI)   // per member on the device: sum log f', then the 3 T + 1 gradient sums

// ---- the front end of every batched entry (api_internal.h, "members") ------------------------------------------------------------
int member_params(const gp_ctx *g, int nb, const double *variance, const double *lengthscale, const double *noise,
                  std::vector<KernParams> *kp) {
    const int D = g->D, nls = g->ard ? D : 1;
    for (int r = 0; r < nb; ++r) {
        if (!(variance[r] > 0.0)) return fail(GP_ERR_ARG, "member %d: variance must be positive", r);
        if (!(noise[r] > 0.0)) return fail(GP_ERR_ARG, "member %d: noise must be positive", r);
        for (int d = 0; d < nls; ++d)
            if (!(lengthscale[(long)r * nls + d] > 0.0)) return fail(GP_ERR_ARG, "member %d: lengthscale must be positive", r);
    }
    kp->assign(nb, g->kp);
    for (int r = 0; r < nb; ++r) {
        (*kp)[r].variance = variance[r];
        for (int d = 0; d < D; ++d) (*kp)[r].ls[d] = g->ard ? lengthscale[(long)r * nls + d] : lengthscale[(long)r * nls];
    }
    return 0;
}

int batch_members(gp_ctx *g, const std::vector<KernParams> &kp, const std::vector<double> &diag, long extra, size_t aux_extra,
                  Members *mp, double **dJit, double **extra_at, signed char **aux_at) {
    Members &m = *mp;
    const long Npad = g->Npad;
    const int R = (int)kp.size(), nt = (int)(Npad / GP_TILE), W = std::min(g->panel_tiles, nt), nJ = (nt + W - 1) / W;
    const long PB = (long)W * GP_TILE;
    m.nb = R;
    m.W = W;
    m.lda = Npad;
    m.sA = (Npad + GP_TILE) * Npad;
    m.sI = (long)nt * GP_TILE * GP_TILE;
    m.sP = (long)nJ * PB * PB;
    m.sV = (long)g->P * Npad;
    m.sT = Npad * Npad;
    m.sS = SCAL_GRAD.off + SCAL_GRAD.len;   // log det, alpha . y and every gradient pass's sums of a member
    const long per = m.sA + m.sI + 2 * m.sP + 2 * m.sV + 2 * m.sT + m.sS + 2;
    int rc;
    if ((rc = g->dBatch.reserve(per * R + extra))) return rc;
    const size_t kp_bytes = (sizeof(KernParams) * R + 255) / 256 * 256, info_bytes = (sizeof(int) * 4 * R + 255) / 256 * 256;
    if ((rc = g->dBatchAux.reserve((long)(aux_extra ? kp_bytes + info_bytes + aux_extra : kp_bytes + sizeof(int) * 4 * R)))) return rc;
    m.A = g->dBatch;
    m.invL = m.A + R * m.sA;
    m.invP = m.invL + R * m.sI;
    m.invPw = m.invP + R * m.sP;
    m.alpha = m.invPw + R * m.sP;
    m.w = m.alpha + R * m.sV;
    m.T = m.Wi = m.w + R * m.sV;        // the identity, then (zeroed) Ky^-1
    m.T2 = m.partial = m.T + R * m.sT;  // L^-T, then the gradient partials (free after the product)
    m.scal = m.T2 + R * m.sT;
    double *dDiag = m.scal + R * m.sS;
    *dJit = dDiag + R;
    *extra_at = *dJit + R;
    KernParams *dKp = (KernParams *)g->dBatchAux.p;
    m.info = (int *)(g->dBatchAux + kp_bytes);
    if (aux_at) *aux_at = g->dBatchAux + kp_bytes + info_bytes;
    m.kp = kp.data();
    m.kpt = dKp;
    m.diag = diag.data();
    m.diag_tab = dDiag;
    m.jit_tab = *dJit;
    // the diagonal-tile kernel writes the lower block triangle of each inverted tile only: the blocks above it must be zero (as
    // set_data leaves the context's dInvL); the buffer is reused across calls of other shapes, so this is per call
    HIPCHK(hipMemsetAsync(m.invL, 0, sizeof(double) * m.sI * R, g->s));
    HIPCHK(hipMemcpyAsync(dKp, kp.data(), sizeof(KernParams) * R, hipMemcpyHostToDevice, g->s));
    HIPCHK(hipMemcpyAsync(dDiag, diag.data(), sizeof(double) * R, hipMemcpyHostToDevice, g->s));
    return 0;
}

// The shared body of the three batch entries: checks, the members over dBatch (batch_members) with the warped models' blocks
// behind them, the per-member jitter ladder (ky_ladder) and the sequence after the factorisation.  `who` names the entry in the
// messages.
static int fit_grad_members(gp_ctx *g, const char *who, int R, const double *variance, const double *lengthscale, const double *noise,
                            int maxtries, double *lml, double *logdet, double *jitter_used, double *dvariance, double *dlengthscale,
                            double *dnoise, int *status, const BatchInputs *bx, const BatchWarp *bw) {
    GP_DEAD_CHECK(g);
    GP_NO_MEAN(g, who);
    GP_NO_LAPLACE(g, who);   // (the members would regress on the labels under the noise of that state)
    if (!g->have_data || !g->have_params) return fail(GP_ERR_STATE, "set data and params before %s", who);
    if (!bx && !bw && g->warp.n > 0)   // the members share Y, and each would need targets warped by parameters of its own
        return fail(GP_ERR_STATE, "gp_fit_grad_batch: an output warp is on (gp_set_output_warp); use gp_fit_grad_warp");
    if (R < 1) return fail(GP_ERR_ARG, "R must be at least 1");
    if (R > GP_BATCH_MAX_R) return fail(GP_ERR_ARG, "%s takes at most R = %d members (got %d)", who, GP_BATCH_MAX_R, R);
    if (g->Npad > GP_BATCH_MAX_NPAD)
        return fail(GP_ERR_ARG, "%s covers Npad <= %d (N = %ld pads to %ld): use %s", who, GP_BATCH_MAX_NPAD, g->N, g->Npad,
                    bx ? "gp_fit_grad_x" : (bw ? "gp_fit_grad_warp" : "gp_fit_grad"));
    if (g->P > GP_GRAD_MAX_P) return fail(GP_ERR_ARG, "%s supports P <= %d", who, GP_GRAD_MAX_P);
    if (bx && g->kp.gower) return fail(GP_ERR_ARG, "%s: not defined for a Gower model", who);   // (as gp_lml_grad_x)
    if (int e = lml_grad_lds_check(g, who)) return e;   // D and P jointly, against the LDS of a workgroup (api_internal.h)
    if (bx)
        if (int e = gradx_lds_check(g, who)) return e;
    if (bw && g->P != 1) return fail(GP_ERR_ARG, "%s: an output warp takes P = 1 (the data has P = %d)", who, g->P);
    if (bw && (bw->n_terms < 1 || bw->n_terms > GP_WARP_MAX_TERMS))
        return fail(GP_ERR_ARG, "%s takes a warp of 1..%d terms", who, GP_WARP_MAX_TERMS);
    const int D = g->D, nls = g->ard ? D : 1;
    std::vector<KernParams> kp;   // per-member parameters
    if (int e = member_params(g, R, variance, lengthscale, noise, &kp)) return e;
    std::vector<WarpParams> wp;
    if (bw) {
        wp.resize(R);
        for (int r = 0; r < R; ++r) {
            WarpParams &w = wp[r];
            memset(&w, 0, sizeof w);
            w.n = bw->n_terms;
            w.d = bw->d[r];
            for (int i = 0; i < w.n; ++i) {
                const double *q = bw->psi + ((long)r * w.n + i) * 3;
                w.a[i] = q[0];
                w.b[i] = q[1];
                w.c[i] = q[2];
            }
            if (!warp_params_valid(w))
                return fail(GP_ERR_ARG, "member %d: warp parameters must be finite with a >= 0, b >= 0 and d > 0", r);
        }
    }
    HIPCHK(hipSetDevice(g->device));

    const long N = g->N, Npad = g->Npad;
    const int P = g->P, nt = (int)(Npad / GP_TILE);
    // behind the plain batch's members: the warp's results and the members' targets, or the members' inputs
    const long sX = bx ? N * D : 0, sY = bw ? Npad : 0, sWo = bw ? GP_BATCH_WARP_OUT : 0;
    // the input-gradient pass puts its partials into the member's T2 block (free once the gradient passes' own partials are
    // summed).  With its rows behind them it would still fit -- (ceil(nt / 4) 16 + D) Npad <= (16 nt + 64) Npad <= 128 nt Npad =
    // Npad^2 for every nt >= 1, Npad = 128 with D = 64 included: 2048 + 8192 of 16384 -- but the rows go to a block of their
    // own, [R, N, D] as the caller wants them, so that they leave in one contiguous copy
    if (bx && gradx_partial_elems(Npad) > Npad * Npad) return fail(GP_ERR_STATE, "%s: the input-gradient partials do not fit a member's block", who);
    std::vector<double> diag(R), diag0(R), jit(R, 0.0);
    for (int r = 0; r < R; ++r) ky_diag(kp[r], noise[r], &diag[r], &diag0[r]);
    Members m;
    double *dJit, *dWarpOut;
    signed char *aux;
    if (int rc = batch_members(g, kp, diag, (2 * sX + sY + sWo) * R, bw ? sizeof(WarpParams) * R : 0, &m, &dJit, &dWarpOut, &aux)) return rc;
    double *dYb = dWarpOut + R * sWo, *dXb = dYb + R * sY, *dGx = dXb + R * sX;
    WarpParams *dWp = bw ? (WarpParams *)aux : nullptr;   // beside kpt: the members' warps
    const double *dYraw = g->warp.n > 0 ? g->dYraw.p : g->dY.p;   // the RAW targets (dY holds f of them while a warp is on)
    m.X = bx ? dXb : g->dX.p;
    m.sX = sX;
    m.Y = bw ? dYb : g->dY.p;
    m.sY = sY;
    m.jit = jit.data();
    if (bx) HIPCHK(hipMemcpyAsync(dXb, bx->Xw, sizeof(double) * sX * R, hipMemcpyHostToDevice, g->s));   // the members' inputs, one copy
    if (bw) {   // the members' targets Y_z = f_z(Y_raw) and sum log f_z'
        HIPCHK(hipMemcpyAsync(dWp, wp.data(), sizeof(WarpParams) * R, hipMemcpyHostToDevice, g->s));
        launch_warp_y_members(g->s, dYraw, N, dWp, dYb, sY, dWarpOut, sWo, R);
    }

    std::vector<int> st(R, 0);
    if (int rc = ky_ladder(g, m, maxtries, diag0, jit, dJit, st)) return rc;

    // everything after the factorisation: all members in the same launches (a failed member's numbers are computed and dropped)
    panel_inv_members(g, m);
    alpha_lml(g, g->s, m);
    identity_blocks(g->s, m.T, Npad, R);
    solve_rows(g, m, nt, 1);   // L^-T into T2
    lauum(g, m);               // Ky^-1 = L^-T (L^-T)^T into Wi
    lml_grad_passes(g, m);
    std::vector<double> sc((size_t)m.sS * R), wo((size_t)sWo * R);
    HIPCHK(hipMemcpyAsync(sc.data(), m.scal, sizeof(double) * m.sS * R, hipMemcpyDeviceToHost, g->s));
    if (bx) {   // dL/dX of every member: partials in its T2 block, its [N, D] rows side by side in dGx
        launch_gradx(g->s, m.X, N, Npad, kp[0], m.alpha, P, m.Wi, Npad, m.T2, dGx, R, m.kpt, m.sX, m.sV, m.sT, m.sT, sX);
        HIPCHK(hipMemcpyAsync(bx->dL_dX, dGx, sizeof(double) * sX * R, hipMemcpyDeviceToHost, g->s));
    }
    if (bw) {
        launch_warp_grad_members(g->s, dYraw, m.alpha, m.sV, N, dWp, dWarpOut + 1, sWo, R);
        HIPCHK(hipMemcpyAsync(wo.data(), dWarpOut, sizeof(double) * sWo * R, hipMemcpyDeviceToHost, g->s));
    }
    GP_SYNC(g->s);

    const double nan = std::nan("");
    const int npsi = bw ? 3 * bw->n_terms : 0;
    for (int r = 0; r < R; ++r) {
        status[r] = st[r];
        if (st[r]) {
            lml[r] = logdet[r] = jitter_used[r] = dvariance[r] = dnoise[r] = nan;
            for (int d = 0; d < nls; ++d) dlengthscale[(long)r * nls + d] = nan;
            if (bx) std::fill(bx->dL_dX + (long)r * sX, bx->dL_dX + (long)(r + 1) * sX, nan);
            if (bw) {
                bw->log_jacobian[r] = bw->dd[r] = nan;
                std::fill(bw->dpsi + (long)r * npsi, bw->dpsi + (long)(r + 1) * npsi, nan);
            }
            continue;
        }
        const double *s = sc.data() + (size_t)m.sS * r;
        logdet[r] = s[SCAL_LOGDET.off];
        lml[r] = lml_from_scalars(N, P, s);
        jitter_used[r] = jit[r];
        grads_from_sums(s + SCAL_GRAD.off, kp[r], g->ard, &dvariance[r], &dlengthscale[(long)r * nls], &dnoise[r]);
        if (bw) {
            const double *o = wo.data() + (size_t)sWo * r;
            bw->log_jacobian[r] = o[0];
            for (int q = 0; q < npsi; ++q) bw->dpsi[(long)r * npsi + q] = o[1 + q];
            bw->dd[r] = o[1 + npsi];
        }
    }
    return 0;
}

extern "C" int gp_fit_grad_batch(gp_t *g, int R, const double *variance, const double *lengthscale, const double *noise, int maxtries,
                                 double *lml, double *logdet, double *jitter_used, double *dvariance, double *dlengthscale,
                                 double *dnoise, int *status) {
    if (!g || !variance || !lengthscale || !noise || !lml || !logdet || !jitter_used || !dvariance || !dlengthscale || !dnoise ||
        !status)
        return fail(GP_ERR_ARG, "null argument");
    return fit_grad_members(g, "gp_fit_grad_batch", R, variance, lengthscale, noise, maxtries, lml, logdet, jitter_used, dvariance,
                            dlengthscale, dnoise, status, nullptr, nullptr);
}

// gp_fit_grad_x for R members over inputs of their own (InputWarpedGP's restarts in lockstep: the caller warps X per member)
extern "C" int gp_fit_grad_x_batch(gp_t *g, int R, const double *Xw, const double *variance, const double *lengthscale,
                                   const double *noise, int maxtries, double *lml, double *logdet, double *jitter_used,
                                   double *dvariance, double *dlengthscale, double *dnoise, double *dL_dX, int *status) {
    if (!g || !Xw || !variance || !lengthscale || !noise || !lml || !logdet || !jitter_used || !dvariance || !dlengthscale || !dnoise ||
        !dL_dX || !status)
        return fail(GP_ERR_ARG, "null argument");
    const BatchInputs bx{Xw, dL_dX};
    return fit_grad_members(g, "gp_fit_grad_x_batch", R, variance, lengthscale, noise, maxtries, lml, logdet, jitter_used, dvariance,
                            dlengthscale, dnoise, status, &bx, nullptr);
}

// gp_fit_grad_warp for R members, each with a tanh warp of its own over the context's raw targets (WarpedGP's restarts in lockstep)
extern "C" int gp_fit_grad_warp_batch(gp_t *g, int R, int n_terms, const double *psi, const double *d, const double *variance,
                                      const double *lengthscale, const double *noise, int maxtries, double *lml, double *logdet,
                                      double *jitter_used, double *dvariance, double *dlengthscale, double *dnoise,
                                      double *log_jacobian, double *dpsi, double *dd, int *status) {
    if (g && (n_terms < 1 || n_terms > GP_WARP_MAX_TERMS))   // (first: a warp of no terms may come with a null psi)
        return fail(GP_ERR_ARG, "gp_fit_grad_warp_batch takes a warp of 1..%d terms", GP_WARP_MAX_TERMS);
    if (!g || !psi || !d || !variance || !lengthscale || !noise || !lml || !logdet || !jitter_used || !dvariance || !dlengthscale ||
        !dnoise || !log_jacobian || !dpsi || !dd || !status)
        return fail(GP_ERR_ARG, "null argument");
    const BatchWarp bw{n_terms, psi, d, log_jacobian, dpsi, dd};
    return fit_grad_members(g, "gp_fit_grad_warp_batch", R, variance, lengthscale, noise, maxtries, lml, logdet, jitter_used,
                            dvariance, dlengthscale, dnoise, status, nullptr, &bw);
}
