// Triangular solves as products with inverted diagonal panels, and Ky^-1 (dtrtri + dpotri re-expressed on the NT GEMM).
// Reference: dtrtrs (posterior.py:294), dpotrs (exact_gaussian_inference.py:60), dpotri (linalg.py:127-145).
#include "api_internal.h"

// ---- inverted diagonal panels ---------------------------------------------------------------------
// invP_J = L_JJ^-1 for every panel J of W tiles (PB = W*128 rows), so that every triangular solve
// against L -- candidates (dtrtrs, posterior.py:294), alpha (dpotrs, exact_gaussian_inference.py:60),
// Ky^-1 (dpotri, linalg.py:127-145) -- is ONE product per panel on the MFMA GEMM instead of a chain of
// W dependent 128-column steps.  Built as the solve of the identity against L_JJ, which gives L_JJ^-T
// (2W-1 small launches), then one transpose.  The GEMM has ONE batch index: the context's build spends
// it on the panels (every launch covers every full panel), the build for several members on the members
// (every launch covers one panel of every member); build_panel_inv_one takes one panel (the factorisation's side stream).

// The solve itself, for diagonal panels of Wp tiles: Wb (PB x PB blocks, the identity on entry) becomes L_JJ^-T.  `o` carries
// the launch's batch and the strides of Wb; sL / sI are those of the panel of L at Lb and of its inverted diagonal tiles at Ib.
void panel_inv_steps(gp_ctx *g, hipStream_t s, double *Wb, long PB, const double *Lb, long lda, const double *Ib, int Wp, GemmOpt o,
                     long sL, long sI) {
    for (int b = 0; b < Wp; ++b) {
        o.inplace = 1;
        o.sB = sI;
        gemm(g, s, 0, Wb, PB, Wb + (long)b * GP_TILE, PB, Ib + (long)b * GP_TILE * GP_TILE, GP_TILE, 0, GP_TILE,
             TileSet{0, b + 1, b, b + 1, 0}, o);
        if (b + 1 < Wp) {
            o.inplace = 0;
            o.sB = sL;
            gemm(g, s, 1, Wb, PB, Wb + (long)b * GP_TILE, PB, Lb + (long)b * GP_TILE, lda, 1, GP_TILE,
                 TileSet{0, b + 1, b + 1, Wp, 0}, o);
        }
    }
}

// room for the inverted diagonal panels of an nt-tile factor in panels of W tiles, and for their build workspace
int reserve_panel_inv(gp_ctx *g, int W, int nt) {
    const long PB = (long)W * GP_TILE, n = (long)((nt + W - 1) / W) * PB * PB;
    const int rc = g->dInvP.reserve(n);
    return rc ? rc : g->dInvPw.reserve(n);
}

void build_panel_inv_one(gp_ctx *g, hipStream_t s, int J, int W, int nt) {
    const long lda = g->Npad;
    const long PB = (long)W * GP_TILE;
    const int J0 = J * W, Wp = std::min(W, nt - J0);
    double *Wb = g->dInvPw + (long)J * PB * PB;
    const double *Lb = g->dA + (long)J * (PB * lda + PB);
    const double *Ib = g->dInvL + (long)J0 * GP_TILE * GP_TILE;
    launch_set_identity_blocks(s, Wb, PB, 1);
    panel_inv_steps(g, s, Wb, PB, Lb, lda, Ib, Wp, GemmOpt(), 0, 0);
    launch_transpose_blocks(s, g->dInvP + (long)J * PB * PB, Wb, PB, 1);
}

int ensure_panel_inv(gp_ctx *g) {
    const long Npad = g->Npad, lda = g->Npad;
    const int nt = (int)(Npad / GP_TILE);
    const int W = std::min(g->panel_tiles, nt);
    // (the width actually built is min(panel_tiles, nt): compared with panel_tiles itself, a matrix of fewer tiles than one
    // panel -- N <= 640 by default, the size of most BO loops -- rebuilt its inverted panel on EVERY predict call: round 4 finding)
    if (g->invp_valid && g->invp_W == W) return 0;
    const long PB = (long)W * GP_TILE;
    const int nJ = (nt + W - 1) / W, nF = nt / W, Wl = nt % W;
    int rc;
    if ((rc = reserve_panel_inv(g, W, nt))) return rc;
    double *Wk = g->dInvPw;
    hipStream_t s = g->s;
    launch_set_identity_blocks(s, Wk, PB, nJ);
    for (int pass = 0; pass < 2; ++pass) {
        // pass 0: the nF full panels as one batch; pass 1: the ragged last panel (Wl tiles)
        const int batch = pass == 0 ? nF : (Wl ? 1 : 0), Wp = pass == 0 ? W : Wl;
        if (batch == 0) continue;
        const long z0 = pass == 0 ? 0 : nF;
        double *Wb = Wk + z0 * PB * PB;
        const double *Lb = g->dA + z0 * (PB * lda + PB);
        const double *Ib = g->dInvL + z0 * (long)W * GP_TILE * GP_TILE;
        GemmOpt o;
        o.batch = batch;
        o.sC = o.sA = PB * PB;
        panel_inv_steps(g, s, Wb, PB, Lb, lda, Ib, Wp, o, PB * lda + PB, (long)W * GP_TILE * GP_TILE);
    }
    launch_transpose_blocks(s, g->dInvP, Wk, PB, nJ);
    g->invp_W = W;
    g->invp_valid = true;
    return 0;
}

// nb identity blocks of n x n, stacked: launch_set_identity_blocks in pieces whose grid stays within 32768 rows
void identity_blocks(hipStream_t s, double *T, long n, int nb) {
    const int per = (int)std::max(1L, 32768 / n);
    for (int b0 = 0; b0 < nb; b0 += per) launch_set_identity_blocks(s, T + (long)b0 * n * n, n, std::min(per, nb - b0));
}

// The same panels (W tiles wide) for m's members, contiguous in m.invP / m.invPw: one panel of every member per launch.
void panel_inv_members(gp_ctx *g, const Members &m) {
    const long lda = m.lda, PB = (long)m.W * GP_TILE;
    const int W = m.W, nt = (int)(g->Npad / GP_TILE), nJ = (nt + W - 1) / W;
    identity_blocks(g->s, m.invPw, PB, m.nb * nJ);
    for (int J = 0; J < nJ; ++J)
        panel_inv_steps(g, g->s, m.invPw + (long)J * PB * PB, PB, m.A + (long)J * (PB * lda + PB), lda,
                        m.invL + (long)J * W * GP_TILE * GP_TILE, std::min(W, nt - J * W), member_opt(m, GemmOpt(), m.sP, m.sP, 0),
                        m.sA, m.sI);
    launch_transpose_blocks(g->s, m.invP, m.invPw, PB, m.nb * nJ);
}

// Row solve  S = T L^-T  for `mt` row tiles of T (row-major, ld = Npad); T is consumed as the running
// right-hand side.  trapezoid = 1: T is block upper-triangular (row tile r is zero left of column tile r:
// the identity, for L^-T), so panel J only touches the row tiles above its end.
// m.T / m.T2 are T / S, m.W the panel width.
// S[:, J] = T[:, J] invP_J^T for `rows` row tiles   (invP_J lower triangular: column tile c contracts k <= c)
static void panel_solve(gp_ctx *g, hipStream_t s, const Members &m, int J, int rows) {
    const long Npad = g->Npad, PB = (long)m.W * GP_TILE;
    const int J0 = J * m.W, J1 = std::min(J0 + m.W, (int)(Npad / GP_TILE));
    GemmOpt o;
    o.k_end_tri = 1;
    o.b_sub = J0;
    gemm(g, s, 0, m.T2, Npad, m.T + (long)J0 * GP_TILE, Npad, m.invP + (long)J * PB * PB, PB, 1, (J1 - J0) * GP_TILE,
         TileSet{0, rows, J0, J1, 0}, member_opt(m, o, m.sT, m.sT, m.sP));
}
// T[:, c0 .. c1) -= S[:, J0 .. J1) L[c0 .. c1, J0 .. J1)^T   (tile columns)
static void rows_update(gp_ctx *g, hipStream_t s, const Members &m, int J0, int J1, int rows, int c0, int c1) {
    gemm(g, s, 1, m.T, g->Npad, m.T2 + (long)J0 * GP_TILE, g->Npad, m.A + (long)J0 * GP_TILE, m.lda, 1, (J1 - J0) * GP_TILE,
         TileSet{0, rows, c0, c1, 0}, member_opt(m, GemmOpt(), m.sT, m.sT, m.sA));
}
// One step of the solve on stream s: panel J's product with its inverted diagonal panel, then the update of everything right
// of it.  (solve_rows's unpaired step, and a pipelined stage of the look-ahead factorisation, whose caller sets m.W itself.)
void solve_step(gp_ctx *g, hipStream_t s, const Members &m, int J, int rows) {
    const int nt = (int)(g->Npad / GP_TILE), J0 = J * m.W, J1 = std::min(J0 + m.W, nt);
    panel_solve(g, s, m, J, rows);
    if (J1 < nt) rows_update(g, s, m, J0, J1, rows, J1, nt);
}

void solve_rows(gp_ctx *g, const Members &m, int mt, int trapezoid, int J_from) {
    const int nt = (int)(g->Npad / GP_TILE), W = m.W;
    hipStream_t s = g->s;
    for (int J = J_from; J * W < nt;) {
        const int J0 = J * W, J1 = std::min(J0 + W, nt), J2 = std::min(J1 + W, nt);
        const int rows = trapezoid ? std::min(mt, J1) : mt;
        // Two panels per update (full row sets only): panel J+1's columns take panel J's update as a small launch of
        // their own, then ONE launch contracts both panels (K = 2 PB) into everything right of them -- half the round
        // trips of the running right-hand side through HBM and a contraction twice as long.  The accumulator sees the
        // same products in the same order as with one launch per panel: bitwise the same result.
        const bool two = g->pair_panels && !trapezoid && J2 > J1 && J2 < nt;
        if (!two) {
            solve_step(g, s, m, J, rows);
            ++J;
            continue;
        }
        panel_solve(g, s, m, J, rows);
        rows_update(g, s, m, J0, J1, rows, J1, J2);
        panel_solve(g, s, m, J + 1, rows);
        rows_update(g, s, m, J0, J2, rows, J2, nt);
        J += 2;
    }
}

// ---- Ky^-1 (potri-equivalent): dtrtri + dlauum re-expressed on the NT GEMM -------------------------
// W = L^-T is the candidate solve applied to the identity (row c of W = (L^-1 e_c)^T); rows above
// the current panel are still zero, so the tile sets are trapezoids and the cost is N^3/3.
// Ky^-1 = W W^T with the contraction of tile row a starting at column a*128: another N^3/3.
// Reference: pdinv / dpotri (GPy/GPy/util/linalg.py:127-145,193-214), Posterior.woodbury_inv
// (posterior.py:176-196).
// Ky^-1 from m.T2 = L^-T (block upper triangular) into m.Wi
void lauum(gp_ctx *g, const Members &m) {
    const long Npad = g->Npad;
    const int nt = (int)(Npad / GP_TILE);
    hipStream_t s = g->s;
    GemmOpt o;
    o.k_tri = 1;
    if (g->lauum_panels) {
        // Ky^-1 = (L^-T)(L^-T)^T accumulated k-panel by k-panel: panel p (W tiles of k) adds to the tiles (i, c), c <= i,
        // with i below the panel's end.  Every tile of a launch then walks the SAME k range, so the workgroups of an
        // XCD share their operand panels in L2 like the trailing updates do; as one launch over k = i*128 .. N each
        // tile streams its own up-to-33 MB row panels at its own offset and the product runs at the fabric's pace
        // (47 TFLOP/s at N = 32768).  The accumulator holds -Ky^-1 (C -= A B^T is the kernel's update form).
        GP_NOTE(hipMemsetAsync(m.Wi, 0, sizeof(double) * (Npad * Npad + (m.nb - 1) * m.sT), s));   // (members are contiguous)
        const int W = g->panel_tiles;
        for (int k0 = 0; k0 < nt; k0 += W) {
            const int k1 = std::min(k0 + W, nt);
            o.k_sub = k0;
            gemm(g, s, 1, m.Wi, Npad, m.T2 + (long)k0 * GP_TILE, Npad, m.T2 + (long)k0 * GP_TILE, Npad, 1, (k1 - k0) * GP_TILE,
                 TileSet{0, k1, 0, k1, 1}, member_opt(m, o, m.sT, m.sT, m.sT));
        }
        launch_symmetrize_scale(s, m.Wi, Npad, Npad, -1.0, m.nb, m.sT);
    } else {
        gemm(g, s, 0, m.Wi, Npad, m.T2, Npad, m.T2, Npad, 1, (int)Npad, TileSet{0, nt, 0, nt, 1}, member_opt(m, o, m.sT, m.sT, m.sT));
        launch_symmetrize(s, m.Wi, Npad, Npad, m.nb, m.sT);
    }
}

// ... for the context's own fit, as a phase
int wi_lauum(gp_ctx *g) {
    const int ph = phase_begin(g, "potri_lauum", (double)g->N * g->N * g->N / 3.0, 0.0);
    lauum(g, ctx_members(g));
    phase_end(g, ph);
    return 0;
}

int ensure_wi(gp_ctx *g) {
    if (g->wi_valid) return 0;
    if (!g->fitted) return fail(GP_ERR_STATE, "gp_fit first");
    const long Npad = g->Npad;
    const int nt = (int)(Npad / GP_TILE);
    int rc;
    if ((rc = ensure_panel_inv(g))) return rc;
    if ((rc = g->dT.reserve(Npad * Npad))) return rc;
    if ((rc = g->dT2.reserve(Npad * Npad))) return rc;
    if ((rc = g->dWi.reserve(Npad * Npad))) return rc;
    double *T = g->dT;
    hipStream_t s = g->s;
    if (g->emulate_fp64 && g->emulate_fit && g->invp_W % 2 == 0 && !g->lap.on) {   // (a Laplace fit is true fp64 throughout)
        rc = wi_rns(g);
        if (rc == 0) {
            g->wi_valid = true;
            g->predicted = false;
            return 0;
        }
        if (rc != GP_ERR_RANGE) return rc;
        ++g->emu_fallbacks;   // non-finite factor: the true-fp64 path below returns what the reference would
        g->nphases = 0;
    }
    if (g->li_valid && !g->w_in_t2) {
        // the inverse factor of this fit is at hand (ensure_linv, the fused one-row path): L^-T is its transpose, N^2 traffic
        // instead of the N^3 / 3 solve
        int ph = phase_begin(g, "potri_transpose", 0.0, 16.0 * (double)g->N * g->N / 2);
        launch_transpose_tri(s, g->dT2, g->dLi, Npad, 1);
        phase_end(g, ph);
    } else if (!g->w_in_t2) {
        int ph = phase_begin(g, "potri_solve", (double)g->N * g->N * g->N / 3.0, 0.0);
        launch_set_identity(s, T, Npad, Npad);
        solve_rows(g, ctx_members(g), nt, 1);  // dT2 = L^-T (block upper triangular)
        phase_end(g, ph);
    }
    g->w_in_t2 = true;
    if ((rc = wi_lauum(g))) return rc;
    g->wi_valid = true;
    g->predicted = false;  // dT was reused
    return 0;
}

// ---- the explicit inverse factor Li = L^-1 (dtrtri, linalg.py:217-227) for the fused one-row path (onerow.hip) -------------------
// The same solve of the identity as Ky^-1 starts with, kept: lower triangular, row-major, exact zeros above the diagonal.  Half of
// the potri-equivalent's work (no W W^T product) -- all the acquisition optimiser's gradient calls need between two fits.
int ensure_linv(gp_ctx *g) {
    if (g->li_valid) return 0;
    if (!g->fitted) return fail(GP_ERR_STATE, "gp_fit first");
    const long Npad = g->Npad;
    const int nt = (int)(Npad / GP_TILE);
    int rc;
    if ((rc = ensure_panel_inv(g))) return rc;
    if ((rc = g->dT.reserve(Npad * Npad))) return rc;
    if ((rc = g->dT2.reserve(Npad * Npad))) return rc;
    if ((rc = g->dLi.reserve(Npad * Npad))) return rc;
    if (!g->w_in_t2) {
        int ph = phase_begin(g, "potri_solve", (double)g->N * g->N * g->N / 3.0, 0.0);
        launch_set_identity(g->s, g->dT, Npad, Npad);
        solve_rows(g, ctx_members(g), nt, 1);  // dT2 = L^-T (true fp64 in either arithmetic mode)
        phase_end(g, ph);
        g->w_in_t2 = true;
        g->predicted = false;  // dT was reused
    }
    launch_transpose_tri(g->s, g->dLi, g->dT2, Npad, 0);
    g->li_valid = true;
    ++g->linv_builds;
    return 0;
}

extern "C" int gp_get_woodbury_inv(gp_t *g, double *Wi) {
    if (!g || !Wi) return fail(GP_ERR_ARG, "null argument");
    GP_DEAD_CHECK(g);
    HIPCHK(hipSetDevice(g->device));
    int rc;
    if ((rc = ensure_wi(g))) return rc;
    GP_SYNC(g->s);
    HIPCHK(hipMemcpy2D(Wi, sizeof(double) * g->N, g->dWi, sizeof(double) * g->Npad, sizeof(double) * g->N, g->N,
                       hipMemcpyDeviceToHost));
    return 0;
}
