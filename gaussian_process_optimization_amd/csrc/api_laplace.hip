// GP classification: a Bernoulli likelihood with a probit link under Laplace's approximation (Rasmussen & Williams, Algorithms 3.1
// and 5.1; the reference's statement: GPy/inference/latent_function_inference/laplace.py:148-353, likelihoods/bernoulli.py).
//
// The Newton iteration runs in a = K^-1 f.  Each step, on the device: the sites at f (W, g, b = W f + g), rhs = W^1/2 K b, the
// scaling pass B = I + W^1/2 K W^1/2 into dA with rhs in the right-hand-side row, the context's own factorisation B = L L^T
// (single-stream or look-ahead, whichever gp_fit takes at that N; the forward solve rides in the RHS row), the backward solve,
// a_new = b - W^1/2 B^-1 rhs, and ONE product K (a_new - a): f is linear in a, so every trial step of the halving reads it.
// The host reads one small block per step (objective, norms, pivot status, log|B|) to decide on halving and stopping.
//
// K is built ONCE per call (launch_kbuild, full, no noise and no 1e-8) and kept in a buffer of its own beside dA: a second
// Npad x Npad matrix, 8 Npad^2 bytes (2.1 GB at N = 16384).  Regenerating K where it is consumed would cost one covariance
// evaluation per entry in the scaling pass and in both products of every step, 3 x (5 ... 11) passes against one.
//
// What is left behind is an exact GP in disguise: (K + W^-1)^-1 = W^1/2 B^-1 W^1/2, so diag(W^-1/2) L is the lower factor of
// K + W^-1.  The context keeps that factor in dA, a in dAlpha, L~^T a in the RHS row and noise 1 -- gp_predict*, the rows entries,
// the candidate tables and the feasibility fold answer with the latent posterior, with include_noise its variance + 1, which is
// what the probit predictive Phi(m / sqrt(1 + s^2)) takes.
#include "api_internal.h"

namespace {

// Any error return after work was forked onto the side streams leaves them joined (as fit_impl's guard)
struct LapQuiesce {
    gp_ctx *g;
    bool armed = true;
    ~LapQuiesce() {
        if (!armed) return;
        for (hipStream_t st : {g->s_panel, g->s_bulk, g->s_inv, g->s_pred, g->s})
            if (st) hipStreamSynchronize(st);
    }
};

inline double *vec(gp_ctx *g, int k) { return g->lap.dVec + (long)k * g->Npad; }

// one factorisation of what dA holds, RHS row included; the inverted diagonal panels afterwards
int lap_factor(gp_ctx *g) {
    const int nt = (int)(g->Npad / GP_TILE);
    g->lr_valid = false;
    g->invp_valid = false;
    g->jitter_try = 0.0;
    HIPCHK(hipMemsetAsync(g->dInfo, 0, sizeof(int) * 4, g->s));
    const bool la = g->lookahead && nt > g->panel_tiles && nt > g->lookahead_min_tiles;   // gp_fit's rule (factor_attempt)
    int rc;
    if ((rc = la ? factor_lookahead(g) : factor(g))) return rc;
    return ensure_panel_inv(g);
}

struct LapOut { double logz = 0.0, logdet = 0.0; int iters = 0, halvings = 0, converged = 0; };

int lap_preamble(gp_ctx *g, const double *labels, int max_iter, const char *who) {
    if (!g->have_data || !g->have_params) return fail(GP_ERR_STATE, "set data and params before %s", who);
    if (g->P != 1) return fail(GP_ERR_STATE, "%s needs P == 1 (one column of labels)", who);
    if (g->kp.gower) return fail(GP_ERR_STATE, "%s: not available for a Gower kernel", who);
    if (g->warp.n > 0) return fail(GP_ERR_STATE, "%s: an output warp is on", who);
    GP_NO_MEAN(g, who);
    if (max_iter < 1 || max_iter > GP_LAPLACE_MAX_ITER) return fail(GP_ERR_ARG, "%s: max_iter out of range (1..%d)", who, GP_LAPLACE_MAX_ITER);
    for (long i = 0; i < g->N; ++i)
        if (labels[i] != 1.0 && labels[i] != -1.0) return fail(GP_ERR_ARG, "%s: label %ld is %g, not -1 or +1", who, i, labels[i]);
    return 0;
}

// The fit.  Stopping rule: the accepted step s da is at most 1e-10 of max |a|, or the objective has not moved by more than 1e-13
// of its size for the second step in a row (Newton converges quadratically: the first such step was ~3e-7 of a, the second is
// at the rounding floor).  Either way W -- evaluated BEFORE the last step -- is within ~1e-10 of W at the mode.
int lap_fit(gp_ctx *g, const double *labels, int max_iter, LapOut *o) {
    HIPCHK(hipSetDevice(g->device));
    LapQuiesce guard{g};
    const long N = g->N, Npad = g->Npad;
    LapState &L = g->lap;
    int rc;
    fit_dropped(g);
    g->nphases = 0;
    g->emu_off_call = true;   // true fp64 throughout: option "emulate_fp64" does not apply
    L.iters = L.halvings = 0;
    if ((rc = L.dK.reserve(Npad * Npad))) return rc;
    if ((rc = L.dVec.reserve((long)LAP_NVEC * Npad))) return rc;
    if ((rc = L.dRes.reserve(2 * LAP_RES_DOUBLES))) return rc;
    hipStream_t s = g->s;
    HIPCHK(hipMemsetAsync(L.dVec, 0, sizeof(double) * LAP_NVEC * Npad, s));
    HIPCHK(hipMemcpyAsync(vec(g, LAP_Y), labels, sizeof(double) * N, hipMemcpyHostToDevice, s));
    launch_kbuild(s, L.dK, Npad, g->dX, N, Npad, g->kp, 0.0, 1);
    double *A = g->dA, *rhs_row = g->dA + Npad * Npad;
    double psi_old = (double)N * std::log(0.5), res[LAP_RES_DOUBLES], logdet = 0.0;
    int info = 0, stalls = 0;
    bool line_search_failed = false;
    auto read_step = [&](bool all) -> int {
        HIPCHK(hipMemcpyAsync(res, L.dRes, sizeof(double) * LAP_RES_DOUBLES, hipMemcpyDeviceToHost, s));
        if (all) {
            HIPCHK(hipMemcpyAsync(&info, g->dInfo, sizeof(int), hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(&logdet, g->dScal + SCAL_LOGDET.off, sizeof(double), hipMemcpyDeviceToHost, s));
        }
        GP_SYNC(s);
        return 0;
    };
    for (int it = 1; it <= max_iter; ++it) {
        launch_lap_site(s, vec(g, LAP_Y), vec(g, LAP_F), N, Npad, vec(g, LAP_W), vec(g, LAP_SW), vec(g, LAP_B), vec(g, LAP_T));
        launch_lap_matvec(s, L.dK, Npad, vec(g, LAP_B), N, vec(g, LAP_SW), nullptr, vec(g, LAP_RHS));
        launch_lap_bbuild(s, A, Npad, L.dK, Npad, vec(g, LAP_SW), N, Npad);
        launch_set_rhs(s, A, Npad, vec(g, LAP_RHS), N, Npad, 1, 1, 0, 0);
        if ((rc = lap_factor(g))) return rc;
        launch_logdet(s, A, Npad, N, g->dScal + SCAL_LOGDET.off);
        launch_trsv_backward(s, A, Npad, g->dInvP, g->invp_W, Npad, rhs_row, Npad, 1, vec(g, LAP_SOL), g->dW);
        launch_lap_dir(s, vec(g, LAP_B), vec(g, LAP_SW), vec(g, LAP_SOL), vec(g, LAP_A), N, Npad, vec(g, LAP_DA));
        launch_lap_matvec(s, L.dK, Npad, vec(g, LAP_DA), N, nullptr, nullptr, vec(g, LAP_DF));
        double step = 1.0;
        launch_lap_psi(s, vec(g, LAP_Y), vec(g, LAP_A), vec(g, LAP_DA), vec(g, LAP_F), vec(g, LAP_DF), step, N, L.dRes);
        if ((rc = read_step(true))) return rc;
        L.iters = it;
        if (info != 0) {   // B has eigenvalues >= 1: a failed pivot means non-finite inputs or parameters.  No jitter ladder
            g_err = "gp_laplace_fit: B = I + W^1/2 K W^1/2 is not positive definite";
            o->iters = it;
            o->halvings = L.halvings;
            return info > 0 ? info : 1;
        }
        // halve while the objective decreases (concave for the probit: the full step is almost always taken); a non-decrease
        // within rounding is accepted
        const double tol = 1e-12 * std::max(1.0, std::fabs(psi_old));
        int halv = 0;
        while (!(res[0] >= psi_old - tol) && halv < 30) {
            step *= 0.5;
            ++halv;
            launch_lap_psi(s, vec(g, LAP_Y), vec(g, LAP_A), vec(g, LAP_DA), vec(g, LAP_F), vec(g, LAP_DF), step, N, L.dRes);
            if ((rc = read_step(false))) return rc;
        }
        L.halvings += halv;
        if (!(res[0] >= psi_old - tol)) {        // no step length helps (a NaN objective included)
            line_search_failed = true;
            break;
        }
        launch_lap_accept(s, vec(g, LAP_A), vec(g, LAP_DA), vec(g, LAP_F), vec(g, LAP_DF), step, N);
        const bool small = step * res[3] <= 1e-10 * res[4];
        stalls = std::fabs(res[0] - psi_old) <= 1e-13 * std::max(1.0, std::fabs(psi_old)) ? stalls + 1 : 0;
        psi_old = res[0];
        if (small || stalls >= 2) {
            o->converged = 1;
            break;
        }
    }
    o->iters = L.iters;
    o->halvings = L.halvings;
    if (!o->converged) {
        g_err = line_search_failed
                    ? "gp_laplace_fit: the line search failed: 30 halvings of the Newton step did not stop the objective from decreasing (a non-finite objective included)"
                    : "gp_laplace_fit: the Newton iteration did not converge within max_iter steps";
        return GP_LAPLACE_NOT_CONVERGED;
    }
    // the Laplace-fitted state: the factor of K + W^-1, a, L~^T a in the RHS row, noise 1
    launch_lap_wrange(s, vec(g, LAP_W), N, L.dRes + LAP_RES_DOUBLES);
    launch_lap_scale_factor(s, A, Npad, g->dInvL, vec(g, LAP_SW), N, Npad);
    launch_lap_ltvec(s, A, Npad, vec(g, LAP_A), N, Npad, rhs_row);
    HIPCHK(hipMemcpyAsync(g->dAlpha, vec(g, LAP_A), sizeof(double) * Npad, hipMemcpyDeviceToDevice, s));
    double wr[2];
    HIPCHK(hipMemcpyAsync(wr, L.dRes + LAP_RES_DOUBLES, sizeof(double) * 2, hipMemcpyDeviceToHost, s));
    GP_SYNC(s);
    g->invp_valid = false;   // the panels built beside the factorisation are those of L, not of diag(W^-1/2) L
    L.wmin = wr[0];
    L.wmax = wr[1];
    o->logdet = logdet;
    o->logz = (res[1] + res[2]) - 0.5 * logdet;
    g->lml = o->logz;
    g->logdet = logdet;
    g->jitter = 0.0;
    L.noise_saved = g->noise;
    g->noise = 1.0;
    L.on = true;
    g->fitted = true;
    guard.armed = false;
    return 0;
}

// d log Z / d (variance, lengthscales) of the fit just made: R = (K + W^-1)^-1 as ensure_wi builds Ky^-1, the vectors s2 and u,
// and the tile pass with the weights 1/2 (a a^T + a u^T + u a^T - R)
int lap_grad(gp_ctx *g, double *grad) {
    const long N = g->N, Npad = g->Npad;
    LapState &L = g->lap;
    hipStream_t s = g->s;
    int rc;
    if ((rc = ensure_wi(g))) return rc;
    launch_lap_s2(s, g->dWi, Npad, vec(g, LAP_W), vec(g, LAP_T), N, Npad, vec(g, LAP_S2));
    launch_lap_matvec(s, L.dK, Npad, vec(g, LAP_S2), N, nullptr, nullptr, vec(g, LAP_TMP));
    launch_lap_matvec(s, g->dWi, Npad, vec(g, LAP_TMP), N, nullptr, vec(g, LAP_S2), vec(g, LAP_U));   // u = s2 - R K s2
    HIPCHK(hipMemcpyAsync(vec(g, LAP_AU), vec(g, LAP_A), sizeof(double) * Npad, hipMemcpyDeviceToDevice, s));
    int pass = 0;
    for (int d0 = 0; d0 < g->D; d0 += GP_GRAD_CH, ++pass) {   // (per-tile partials in dT: free once R is in dWi)
        launch_lap_grad(s, g->dX, N, Npad, g->kp, g->ard, d0, vec(g, LAP_AU), g->dWi, Npad, g->dT,
                        g->dScal + SCAL_GRAD.off + pass * GP_GRAD_NACC);
        if (!g->ard) break;
    }
    const int npass = g->ard ? (g->D + GP_GRAD_CH - 1) / GP_GRAD_CH : 1;
    std::vector<double> host((size_t)GP_GRAD_NACC * npass);
    HIPCHK(hipMemcpyAsync(host.data(), g->dScal + SCAL_GRAD.off, sizeof(double) * host.size(), hipMemcpyDeviceToHost, s));
    GP_SYNC(s);
    double dnoise = 0.0;   // (the probit has no likelihood parameter)
    grads_from_sums(host.data(), g->kp, g->ard, grad, grad + 1, &dnoise);
    return 0;
}

void lap_out(const LapOut &o, double *logz, double *logdet_b, int *iters, int *halvings, int *converged) {
    if (logz) *logz = o.logz;
    if (logdet_b) *logdet_b = o.logdet;
    if (iters) *iters = o.iters;
    if (halvings) *halvings = o.halvings;
    if (converged) *converged = o.converged;
}

}   // namespace

extern "C" int gp_laplace_fit(gp_t *g, const double *labels, int max_iter, double *logz, double *logdet_b, int *iters, int *halvings,
                              int *converged) {
    if (!g || !labels) return fail(GP_ERR_ARG, "null argument");
    GP_DEAD_CHECK(g);
    int rc;
    if ((rc = lap_preamble(g, labels, max_iter, "gp_laplace_fit"))) return rc;
    LapOut o;
    rc = lap_fit(g, labels, max_iter, &o);
    lap_out(o, logz, logdet_b, iters, halvings, converged);
    return rc;
}

extern "C" int gp_laplace_fit_grad(gp_t *g, const double *labels, int max_iter, double *logz, double *logdet_b, int *iters,
                                   int *halvings, int *converged, double *grad) {
    if (!g || !labels || !grad) return fail(GP_ERR_ARG, "null argument");
    GP_DEAD_CHECK(g);
    int rc;
    if ((rc = lap_preamble(g, labels, max_iter, "gp_laplace_fit_grad"))) return rc;
    const size_t need = lml_grad_lds_bytes(g->D, 0, 2);   // before the fit: a refused call leaves the context as it was
    if (need > (size_t)g->lds_per_wg)
        return fail(GP_ERR_ARG, "gp_laplace_fit_grad: D = %d needs %zu bytes of LDS per workgroup in the gradient pass, the device has %ld",
                    g->D, need, g->lds_per_wg);
    LapOut o;
    rc = lap_fit(g, labels, max_iter, &o);
    lap_out(o, logz, logdet_b, iters, halvings, converged);
    return rc ? rc : lap_grad(g, grad);
}

extern "C" int gp_laplace_info(gp_t *g, int *iters, int *halvings, double *wmin, double *wmax) {
    if (!g) return fail(GP_ERR_ARG, "null gp");
    GP_DEAD_CHECK(g);
    if (!g->lap.on) return fail(GP_ERR_STATE, "gp_laplace_info: the handle is not Laplace-fitted (gp_laplace_fit)");
    if (iters) *iters = g->lap.iters;
    if (halvings) *halvings = g->lap.halvings;
    if (wmin) *wmin = g->lap.wmin;
    if (wmax) *wmax = g->lap.wmax;
    return 0;
}

extern "C" int gp_laplace_get_mode(gp_t *g, double *f, double *W) {
    if (!g) return fail(GP_ERR_ARG, "null gp");
    GP_DEAD_CHECK(g);
    if (!g->lap.on) return fail(GP_ERR_STATE, "gp_laplace_get_mode: the handle is not Laplace-fitted (gp_laplace_fit)");
    HIPCHK(hipSetDevice(g->device));
    GP_SYNC(g->s);
    if (f) HIPCHK(hipMemcpy(f, vec(g, LAP_F), sizeof(double) * g->N, hipMemcpyDeviceToHost));
    if (W) HIPCHK(hipMemcpy(W, vec(g, LAP_W), sizeof(double) * g->N, hipMemcpyDeviceToHost));
    return 0;
}
