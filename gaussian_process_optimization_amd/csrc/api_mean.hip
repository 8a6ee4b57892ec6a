// The mean function of the exact GP: GPRegression(..., mean_function=...) over GPy's mappings.Linear, mappings.Constant and their
// Additive sum (core/gp.py:89-95: the mapping is a parameter of the model; :267-271: its gradients from dL_dm = alpha; :293-294: it is
// added to the posterior mean; exact_gaussian_inference.py:42-50: the fit runs on Y - m(X)).  The handle keeps a snapshot of A and b
// and the kernels of csrc/mean.hip; see include/gphip.h for the contract of each entry point.
#include "api_internal.h"

// dY <- dYraw - m(X) where the data or the mean changed since dY was last built.  Drained, so that every stream of the
// factorisation that follows finds the residuals there.
int mean_residuals(gp_ctx *g) {
    MeanState &mf = g->mean;
    if (!mf.on() || !mf.stale) return 0;
    launch_mean_residual(g->s, g->dX, g->dYraw, g->N, g->D, g->P, mf.dAb, g->dY);
    GP_SYNC(g->s);
    mf.stale = false;
    return 0;
}

void mean_add(gp_ctx *g, const double *X, long M, double *mean) {
    if (g->mean.on()) launch_mean_add(g->s, X, M, g->D, g->P, g->mean.dAb, mean);
}

void mean_add_grad(gp_ctx *g, long M, double *dmdx) {
    if (g->mean.has_A) launch_mean_add_grad(g->s, M, g->D, g->P, g->mean.dAb, dmdx);
}

extern "C" int gp_mean_set(gp_t *g, const double *A, const double *b) {
    if (!g) return fail(GP_ERR_ARG, "null gp");
    GP_DEAD_CHECK(g);
    if (!g->have_data) return fail(GP_ERR_STATE, "gp_mean_set: gp_set_data first (A is [D, P] and b [P] of the data)");
    GP_NO_LAPLACE(g, "gp_mean_set");
    if (g->warp.n > 0)
        return fail(GP_ERR_STATE, "gp_mean_set: an output warp is on (gp_set_output_warp): a mean function and a warp do not combine");
    MeanState &mf = g->mean;
    const int D = g->D, P = g->P;
    const long nA = (long)D * P;
    for (long i = 0; A && i < nA; ++i)
        if (!std::isfinite(A[i])) return fail(GP_ERR_ARG, "gp_mean_set: A must be finite (entry %ld)", i);
    for (int p = 0; b && p < P; ++p)
        if (!std::isfinite(b[p])) return fail(GP_ERR_ARG, "gp_mean_set: b must be finite (entry %d)", p);
    HIPCHK(hipSetDevice(g->device));
    GP_SYNC(g->s);   // nothing on the stream still reads the parameters or the targets that are about to change
    const long nY = g->N * (long)P;
    if (!A && !b) {   // clear: the raw targets again
        if (mf.on()) HIPCHK(hipMemcpy(g->dY, g->dYraw, sizeof(double) * nY, hipMemcpyDeviceToDevice));
        mf.has_A = mf.has_b = mf.stale = false;
    } else {
        int rc;
        if ((rc = mf.dAb.reserve((long)GP_MAX_D * GP_MAX_RHS + GP_MAX_RHS))) return rc;
        if (!mf.on()) {   // dY still holds the raw targets
            if ((rc = g->dYraw.reserve(g->capN * (long)g->capP))) return rc;
            HIPCHK(hipMemcpy(g->dYraw, g->dY, sizeof(double) * nY, hipMemcpyDeviceToDevice));
        }
        std::vector<double> ab((size_t)nA + P, 0.0);
        if (A) memcpy(ab.data(), A, sizeof(double) * nA);
        if (b) memcpy(ab.data() + nA, b, sizeof(double) * P);
        HIPCHK(hipMemcpy(mf.dAb, ab.data(), sizeof(double) * ab.size(), hipMemcpyHostToDevice));
        mf.has_A = A != nullptr;
        mf.has_b = b != nullptr;
        mf.stale = true;
    }
    fit_dropped(g);   // what gp_set_params drops
    sparse_fit_dropped(g);
    return 0;
}

extern "C" int gp_mean_info(gp_t *g, int *has_A, int *has_b) {
    if (!g) return fail(GP_ERR_ARG, "null gp");
    if (has_A) *has_A = g->mean.has_A ? 1 : 0;
    if (has_b) *has_b = g->mean.has_b ? 1 : 0;
    return 0;
}

extern "C" int gp_mean_grad(gp_t *g, double *dA, double *db) {
    if (!g) return fail(GP_ERR_ARG, "null gp");
    GP_FITTED(g);
    GP_NO_LAPLACE(g, "gp_mean_grad");
    MeanState &mf = g->mean;
    const int D = g->D, P = g->P, nout = (D + 1) * P;
    const long npart = (long)mean_grad_chunks(g->N) * nout;
    int rc;
    if ((rc = mf.dPart.reserve(npart + nout))) return rc;
    double *out = mf.dPart + npart;
    launch_mean_grad(g->s, g->dX, g->dAlpha, g->Npad, g->N, D, P, mf.dPart, out);
    if (dA) HIPCHK(hipMemcpyAsync(dA, out, sizeof(double) * D * P, hipMemcpyDeviceToHost, g->s));
    if (db) HIPCHK(hipMemcpyAsync(db, out + (long)D * P, sizeof(double) * P, hipMemcpyDeviceToHost, g->s));
    GP_SYNC(g->s);
    return 0;
}
