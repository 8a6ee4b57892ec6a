// gp_append: k new rows join the data of a valid fit and the factor grows by them, O(k N^2), instead of being rebuilt (N^3 / 3).
// The factor of [[K11, K12], [K21, K22]] is the old factor with the rows [L21 | L22] under it:
//   T = L11^-1 K(X, Xnew),  S = K(Xnew, Xnew) + (noise + 1e-8 + jitter) I - T^T T,  L22 = chol(S),  L21 = T^T
// (the blocked form of GPy's jitchol, GPy/GPy/util/linalg.py:56-81, applied to the border alone), and where the explicit inverse
// factor is valid it grows too: Li21 = -L22^-1 (L21 Li11), Li22 = L22^-1.  Nothing of that depends on Y; alpha and the LML are
// recomputed from the grown factor and the new targets (z = L^-1 Y, then alpha_lml as every fit).
//
// Padding rows of Ky, L and L^-1 are rows of the identity (kbuild.hip), so a border that stays inside the last 128-row tile is
// written in place; one that starts a new tile first moves every buffer to the new leading dimension.  A call whose rows would
// cross a tile boundary runs as two borders, one on each side: a border never spans two diagonal tiles, and its k x k
// factorisation is the diagonal-tile kernel (potrf.hip) on a scratch tile.  Each border is computed into scratch and committed
// only after the host has seen its pivots; a second border that fails takes the first one back.  Kernels: append.hip.
#include "api_internal.h"

namespace {

// the border's scratch, carved from g->dApp (every offset even: the kernels load pairs)
struct Border {
    long ldt;          // leading dimension of the k-row blocks: the Npad the border was computed under
    double *xn;        // [k, D] the new inputs
    double *kx;        // [k, ldt] K(Xnew, X) (consumed by the substitution route)
    double *t;         // [k, ldt] T^T = L21
    double *r;         // [k, ldt] L21 Li11, then (over kx) Li21
    double *part;      // partials of the column sums
    double *gpart;     // partials of the Gram
    double *knn, *s, *sinv, *rt, *invb;   // tiles: K(Xnew, Xnew); S -> L22; L22^-1; L21 InvL_t and the new rows of the inverted tile
};

int border_scratch(gp_ctx *g, int k, Border *b) {
    const long ldt = g->Npad, T2 = (long)GP_TILE * GP_TILE;
    const long n_x = round_up((long)k * g->D, 2), n_k = (long)k * ldt;
    const long n_part = (long)append_col_chunks(g->N) * GP_APPEND_V * ldt + GP_APPEND_V * GP_TILE;
    const long n_g = round_up(append_gram_elems(g->N, k), 2);
    int rc;
    if ((rc = g->dApp.reserve(n_x + 3 * n_k + n_part + n_g + 5 * T2))) return rc;
    double *p = g->dApp;
    b->ldt = ldt;
    b->xn = p, p += n_x;
    b->kx = p, p += n_k;
    b->t = p, p += n_k;
    b->r = p, p += n_k;
    b->part = p, p += n_part;
    b->gpart = p, p += n_g;
    for (double **q : {&b->knn, &b->s, &b->sinv, &b->rt, &b->invb}) *q = p, p += T2;
    return 0;
}

inline int nt_loads(const gp_ctx *g) { return g->rows_nt < 0 ? (g->Npad > 8192 ? 1 : 0) : g->rows_nt; }   // as the one-location kernels (api_rows.hip)

// The border of k rows Xn (host) under the context's N rows, all inside diagonal tile N / 128, into scratch.  *pivot: 0, or the
// 1-based row of the grown matrix whose pivot was not positive (or not finite).  The context is only read.
int border_compute(gp_ctx *g, const double *Xn, int k, Border *b, long *pivot) {
    const long N = g->N, Npad = g->Npad;
    int rc;
    if ((rc = border_scratch(g, k, b))) return rc;
    hipStream_t s = g->s;
    const int ph = phase_begin(g, "append_border", 2.0 * (double)N * N * k, (g->li_valid ? (k + GP_APPEND_V - 1) / GP_APPEND_V : 1) * 4.0 * (double)N * N);
    HIPCHK(hipMemcpyAsync(b->xn, Xn, sizeof(double) * k * g->D, hipMemcpyHostToDevice, s));
    for (int c = 0; c < k; c += GP_APPEND_V)
        launch_cross_k_rows(s, b->kx + c * Npad, Npad, b->xn + (long)c * g->D, std::min(GP_APPEND_V, k - c), g->dX, N, Npad, g->kp);
    if (g->li_valid) {   // T^T = Kx Li^T: one read of the inverse factor per GP_APPEND_V rows
        HIPCHK(hipMemsetAsync(b->t, 0, sizeof(double) * k * Npad, s));
        for (int c = 0; c < k; c += GP_APPEND_V)
            launch_append_rowdot(s, g->dLi, Npad, N, Npad, b->kx + c * Npad, Npad, std::min(GP_APPEND_V, k - c), b->t + c * Npad, Npad,
                                 nt_loads(g));
    } else {             // by substitution against L (smallm.hip); the inverse factor is not built for this
        if ((rc = ensure_panel_inv(g))) return rc;
        launch_small_forward_solve(s, g->dA, Npad, g->dInvP, g->invp_W, Npad, b->kx, b->t, Npad, k);
    }
    launch_cross_k(s, b->knn, GP_TILE, b->xn, k, GP_TILE, b->xn, k, GP_TILE, g->kp);
    double diag_add, diag0;
    ky_diag(g->kp, g->noise, &diag_add, &diag0);
    HIPCHK(hipMemsetAsync(g->dInfo, 0, sizeof(int) * 4, s));
    HIPCHK(hipMemsetAsync(b->sinv, 0, sizeof(double) * GP_TILE * GP_TILE, s));   // the tile kernel writes the lower block triangle only
    launch_append_schur(s, b->t, Npad, N, k, b->gpart, b->knn, g->kp.variance, g->kp.gower, diag_add, g->jitter, b->s, g->dInfo + 1);
    launch_potrf_tile(s, b->s, GP_TILE, 0, b->sinv, g->dInfo);
    phase_end(g, ph);
    int info[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(info, g->dInfo, sizeof(info), hipMemcpyDeviceToHost, s));
    GP_SYNC(s);
    *pivot = info[1] ? N + 1 : (info[0] > 0 ? N + std::min(info[0], k) : 0);
    return 0;
}

template <class T>
void take(DevBuf<T> &dst, DevBuf<T> &src) {
    std::swap(dst.p, src.p);
    std::swap(dst.cap, src.cap);
}

// One more tile: every buffer of gp_set_data at the new Npad, L (and L^-1 when valid) moved to the new leading dimension with
// strided copies, the new tile's rows the identity.  capN grows as in gp_set_data; the candidates are not touched.
int relayout(gp_ctx *g) {
    const long N = g->N, Np0 = g->Npad, Np1 = Np0 + GP_TILE, T2 = (long)GP_TILE * GP_TILE;
    const int capP = g->capP;
    hipStream_t s = g->s;
    DevBuf<double> X, Y, A, I, Al, W, Mu, Li;
    int rc;
    if ((rc = X.reserve(Np1 * GP_MAX_D)) || (rc = Y.reserve(Np1 * capP)) || (rc = A.reserve((Np1 + GP_MAX_RHS) * Np1)) ||
        (rc = I.reserve(Np1 * GP_TILE)) || (rc = Al.reserve(Np1 * capP)) || (rc = W.reserve(Np1 * capP)) || (rc = Mu.reserve(Np1 * 16)))
        return rc;
    if (g->li_valid && (rc = Li.reserve(Np1 * Np1))) return rc;
    HIPCHK(hipMemcpyAsync(X, g->dX, sizeof(double) * N * g->D, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemsetAsync(A, 0, sizeof(double) * (Np1 + GP_MAX_RHS) * Np1, s));
    HIPCHK(hipMemcpy2DAsync(A, sizeof(double) * Np1, g->dA, sizeof(double) * Np0, sizeof(double) * Np0, Np0, hipMemcpyDeviceToDevice, s));
    launch_append_identity_rows(s, A, Np1, Np1, Np0, Np1);
    HIPCHK(hipMemsetAsync(I, 0, sizeof(double) * Np1 * GP_TILE, s));
    HIPCHK(hipMemcpyAsync(I, g->dInvL, sizeof(double) * Np0 * GP_TILE, hipMemcpyDeviceToDevice, s));
    launch_append_identity_rows(s, I + Np0 / GP_TILE * T2, GP_TILE, GP_TILE, 0, GP_TILE);
    if (g->li_valid) {
        HIPCHK(hipMemsetAsync(Li, 0, sizeof(double) * Np1 * Np1, s));
        HIPCHK(hipMemcpy2DAsync(Li, sizeof(double) * Np1, g->dLi, sizeof(double) * Np0, sizeof(double) * Np0, Np0, hipMemcpyDeviceToDevice, s));
        launch_append_identity_rows(s, Li, Np1, Np1, Np0, Np1);
    }
    GP_SYNC(s);
    take(g->dX, X), take(g->dY, Y), take(g->dA, A), take(g->dInvL, I), take(g->dAlpha, Al), take(g->dW, W), take(g->dMu, Mu);
    if (g->li_valid) take(g->dLi, Li);
    g->Npad = g->capN = Np1;
    return 0;   // (the old blocks are freed as the locals leave)
}

// The computed border becomes rows N .. N + k - 1 of L, of the inverted diagonal tile and, where valid, of L^-1; X grows.
int border_commit(gp_ctx *g, const Border &b, int k) {
    const long N = g->N, r0 = N % GP_TILE, T2 = (long)GP_TILE * GP_TILE;
    int rc;
    if (r0 == 0) {
        const int phr = phase_begin(g, "append_relayout", 0.0, (g->li_valid ? 2 : 1) * 24.0 * (double)g->Npad * g->Npad);
        if ((rc = relayout(g))) return rc;
        phase_end(g, phr);
        ++g->append_relayout;
    } else
        ++g->append_in_place;
    const long Npad = g->Npad, t = N / GP_TILE;
    hipStream_t s = g->s;
    const int ph = phase_begin(g, "append_commit", g->li_valid ? 2.0 * (double)N * N * k : 0.0,
                               g->li_valid ? (k + GP_APPEND_V - 1) / GP_APPEND_V * 4.0 * (double)N * N : 0.0);
    if (g->li_valid) {
        for (int c = 0; c < k; c += GP_APPEND_V)
            launch_append_colsum(s, g->dLi, Npad, N, b.ldt, b.t + c * b.ldt, b.ldt, std::min(GP_APPEND_V, k - c), b.part, b.ldt,
                                 b.r + c * b.ldt, b.ldt, nt_loads(g));
        launch_append_negmul(s, b.sinv, b.r, b.ldt, k, N, b.kx, b.ldt);
        launch_append_commit_rows(s, g->dLi, Npad, Npad, N, k, N, b.kx, b.ldt, b.sinv);
    }
    // the inverted diagonal tile: its new rows are the same expression over the tile alone
    double *It = g->dInvL + t * T2;
    if (r0 > 0) {
        for (int c = 0; c < k; c += GP_APPEND_V)
            launch_append_colsum(s, It, GP_TILE, r0, GP_TILE, b.t + c * b.ldt + t * GP_TILE, b.ldt, std::min(GP_APPEND_V, k - c), b.part,
                                 GP_TILE, b.rt + (long)c * GP_TILE, GP_TILE, 0);
        launch_append_negmul(s, b.sinv, b.rt, GP_TILE, k, r0, b.invb, GP_TILE);
    }
    launch_append_commit_rows(s, It, GP_TILE, GP_TILE, r0, k, r0, b.invb, GP_TILE, b.sinv);
    launch_append_commit_rows(s, g->dA, Npad, Npad, N, k, N, b.t, b.ldt, b.s);
    HIPCHK(hipMemcpyAsync(g->dX + N * g->D, b.xn, sizeof(double) * k * g->D, hipMemcpyDeviceToDevice, s));
    phase_end(g, ph);
    g->N = N + k;
    g->invp_valid = false;   // the last inverted panel belongs to the factor without these rows
    return 0;
}

// alpha, log det and the LML of the grown factor and the targets in dY: z = L^-1 Y into the RHS rows, then alpha_lml
int refresh_alpha(gp_ctx *g) {
    const long N = g->N, Npad = g->Npad;
    const int P = g->P;
    hipStream_t s = g->s;
    int rc;
    int ph = phase_begin(g, "append_panel_inv", 0.0, 0.0);
    if ((rc = ensure_panel_inv(g))) return rc;   // (alpha = L^-T z needs the inverted panels either way)
    phase_end(g, ph);
    if ((rc = g->dApp.reserve((long)P * Npad))) return rc;
    double *yr = g->dApp, *z = g->dA + Npad * Npad;
    ph = phase_begin(g, "append_z", 2.0 * (double)N * N * P, 4.0 * (double)N * N);
    launch_append_yrows(s, g->dY, N, P, Npad, yr, Npad);
    if (g->li_valid) {
        HIPCHK(hipMemsetAsync(z, 0, sizeof(double) * P * Npad, s));
        for (int c = 0; c < P; c += GP_APPEND_V)
            launch_append_rowdot(s, g->dLi, Npad, N, Npad, yr + c * Npad, Npad, std::min(GP_APPEND_V, P - c), z + c * Npad, Npad, nt_loads(g));
    } else
        launch_small_forward_solve(s, g->dA, Npad, g->dInvP, g->invp_W, Npad, yr, z, Npad, P);
    phase_end(g, ph);
    ph = phase_begin(g, "alpha_lml", 2.0 * (double)N * N * P, 4.0 * (double)N * N);
    alpha_lml(g, s, ctx_members(g));
    phase_end(g, ph);
    std::vector<double> sc(SCAL_DOT.off + P);
    HIPCHK(hipMemcpyAsync(sc.data(), g->dScal, sizeof(double) * sc.size(), hipMemcpyDeviceToHost, s));
    GP_SYNC(s);
    g->logdet = sc[SCAL_LOGDET.off];
    g->lml = lml_from_scalars(N, P, sc.data());
    return 0;
}

// A committed in-place border of the rows N0 .. is taken back: the rows are padding again, the inverted tile what it was (saved_tile, host).
int border_undo(gp_ctx *g, long N0, const double *saved_tile) {
    const long Npad = g->Npad, T2 = (long)GP_TILE * GP_TILE;
    hipStream_t s = g->s;
    launch_append_identity_rows(s, g->dA, Npad, Npad, N0, Npad);
    if (g->li_valid) launch_append_identity_rows(s, g->dLi, Npad, Npad, N0, Npad);
    HIPCHK(hipMemcpyAsync(g->dInvL + N0 / GP_TILE * T2, saved_tile, sizeof(double) * T2, hipMemcpyHostToDevice, s));
    GP_SYNC(s);
    g->N = N0;
    g->invp_valid = false;   // (built from the grown factor meanwhile)
    --g->append_in_place;
    return 0;
}

}   // namespace

static int append_refused(gp_ctx *g, int code, const char *fmt, long a = 0, long b = 0) {
    ++g->append_refused;
    return fail(code, fmt, a, b);
}

extern "C" int gp_append(gp_t *g, const double *Xnew, int64_t k, const double *Yall, double *lml, double *logdet) {
    if (!g || !Xnew || !Yall) return fail(GP_ERR_ARG, "null argument");
    GP_DEAD_CHECK(g);
    if (g->mean.on())   // the border's right-hand sides would be raw targets beside residuals
        return append_refused(g, GP_ERR_STATE, "gp_append: not available while a mean function is resident (gp_mean_set(NULL, NULL) clears it)");
    if (g->lap.on)   // the border would be that of K + noise, the factor is that of K + W^-1 at a mode the new rows move
        return append_refused(g, GP_ERR_STATE, "gp_append: not available on a Laplace-fitted handle (gp_laplace_fit): refit");
    if (!g->fitted) return append_refused(g, GP_ERR_STATE, "gp_append extends a valid fit: gp_fit first");
    if (g->warp.n > 0) return append_refused(g, GP_ERR_STATE, "gp_append: an output warp is on (its targets are refitted, not appended)");
    if (k < 1 || k > GP_TILE) return append_refused(g, GP_ERR_ARG, "gp_append: k = %ld outside 1..%ld", (long)k, (long)GP_TILE);
    HIPCHK(hipSetDevice(g->device));
    GP_SYNC(g->s);
    g->nphases = 0;
    const long N0 = g->N, T2 = (long)GP_TILE * GP_TILE;
    // rows up to the end of the current tile first, the rest in a new tile
    const long room = g->Npad - N0;
    const int k1 = (int)((room > 0 && room < k) ? room : k), k2 = (int)k - k1;
    int rc;
    long pivot = 0;
    Border b;
    // an error (a failed HIP call) once rows have been committed leaves a factor whose alpha is not its own: the fit is dropped
    auto broken = [g](int code) {
        fit_dropped(g);
        return code;
    };
    if ((rc = border_compute(g, Xnew, k1, &b, &pivot))) return rc;
    if (pivot) {
        ++g->append_refused;
        g_err = "gp_append: the border is not positive definite";
        return (int)pivot;
    }
    std::vector<double> saved;   // what an undo puts back: the inverted diagonal tile as it is now
    if (k2 > 0) {
        saved.resize(T2);
        HIPCHK(hipMemcpy(saved.data(), g->dInvL + N0 / GP_TILE * T2, sizeof(double) * T2, hipMemcpyDeviceToHost));
    }
    if ((rc = border_commit(g, b, k1))) return broken(rc);
    if (k2 > 0) {
        if ((rc = border_compute(g, Xnew + (long)k1 * g->D, k2, &b, &pivot))) return broken(rc);
        if (pivot) {
            if ((rc = border_undo(g, N0, saved.data()))) return broken(rc);
            ++g->append_refused;
            g_err = "gp_append: the border is not positive definite";
            return (int)pivot;
        }
        if ((rc = border_commit(g, b, k2))) return broken(rc);
    }
    factor_grown(g);
    const hipError_t e = hipMemcpyAsync(g->dY, Yall, sizeof(double) * g->N * g->P, hipMemcpyHostToDevice, g->s);
    if (e != hipSuccess) return broken(fail(GP_ERR_HIP, "gp_append: upload of the targets -> %s", hipGetErrorString(e)));
    if ((rc = refresh_alpha(g))) return broken(rc);
    if (lml) *lml = g->lml;
    if (logdet) *logdet = g->logdet;
    return 0;
}

extern "C" int gp_append_stats(gp_t *g, int64_t *in_place, int64_t *relayout_, int64_t *refused) {
    if (!g) return fail(GP_ERR_ARG, "null gp");
    if (in_place) *in_place = g->append_in_place;
    if (relayout_) *relayout_ = g->append_relayout;
    if (refused) *refused = g->append_refused;
    return 0;
}
