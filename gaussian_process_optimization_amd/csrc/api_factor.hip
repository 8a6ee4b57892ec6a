// The factorisation scheduler: blocked right-looking Cholesky with one panel of look-ahead over the per-device streams,
// the pipelined one-call entry points (gp_fit_predict, the fit half of gp_fit_grad) and gp_fit itself.
// Reference: jitchol / pdinv (GPy/GPy/util/linalg.py:56-81,193-214), ExactGaussianInference.inference
// (inference/latent_function_inference/exact_gaussian_inference.py:37-74).
#include "api_internal.h"

// K, the jitter of a repeated attempt (jitchol retries factor (Ky + jitter I): it lands on the assembled diagonal, linalg.py:69)
// and the RHS rows of m's members
void build_ky(gp_ctx *g, const Members &m, bool jittered) {
    launch_kbuild(g->s, m.A, m.lda, m.X, g->N, g->Npad, m.kp[0], m.diag[0], 0, m.nb, m.sA, m.kpt, m.diag_tab, m.sX);
    if (jittered) launch_add_diag(g->s, m.A, m.lda, g->N, m.jit[0], m.nb, m.sA, m.jit_tab);
    launch_set_rhs(g->s, m.A, m.lda, m.Y, g->N, g->Npad, g->P, m.nb, m.sA, m.sY);
}

// ---- blocked right-looking Cholesky (two-level: 128-column steps inside panel_tiles-wide panels) ----
// m.A: nt x nt tiles (lower) plus R1 - nt extra row tiles that ride through the panel solves and updates (the RHS rows)
// side_inv (the model's own factor only): the inverted diagonal panel of each panel is built on the side stream as soon as that
// panel's columns are final, beside the trailing update and the next panel -- one event record per panel on this stream.
// One step of the in-panel factorisation starting at tile column j of a panel that ends at J1; returns the next column.
// Option "inner_tiles" 2 (default 1: measured neutral) takes two columns at a time: the 256 x 256 diagonal block in ONE launch
// (potrf_pair_kernel: both diagonal tiles, the tile between them solved and the second one updated inside), ONE launch that
// solves both tile columns of the rows below (trsm2.hip), ONE K = 256 update of the panel's remaining columns -- three
// dependent launches per 256 columns where the 128-column step takes six, and contractions twice as long.  (One member only:
// the pair kernels have no batched twin.)
static int chain_step(gp_ctx *g, hipStream_t s, const Members &m, int j, int J1, int R1) {
    double *A = m.A, *invL = m.invL;
    const long lda = m.lda;
    if (g->inner_tiles >= 2 && m.nb == 1 && j + 1 < J1 && R1 - (j + 2) >= g->inner_min_rows) {
        launch_potrf_pair(s, A, lda, j, invL, m.info);
        launch_trsm2(s, A, lda, j, invL, j + 2, R1);
        if (j + 2 < J1)
            gemm(g, s, 1, A, lda, A + (long)j * GP_TILE, lda, A + (long)j * GP_TILE, lda, 1, 2 * GP_TILE,
                 TileSet{0, R1, j + 2, J1, 1});
        return j + 2;
    }
    launch_potrf_tile(s, A, lda, j, invL, m.info, m.nb, m.sA, m.sI, 4);
    // panel solve: A[i, j] <- A[i, j] * inv(L_jj)^T for the row tiles below (and the RHS tile)
    gemm(g, s, 0, A, lda, A + (long)j * GP_TILE, lda, invL + (long)j * GP_TILE * GP_TILE, GP_TILE, 0, GP_TILE,
         TileSet{j + 1, R1, j, j + 1, 0}, member_opt(m, inplace_opt(), m.sA, m.sA, m.sI));
    // update of the remaining columns of this panel (K = 128)
    if (j + 1 < J1)
        gemm(g, s, 1, A, lda, A + (long)j * GP_TILE, lda, A + (long)j * GP_TILE, lda, 1, GP_TILE, TileSet{0, R1, j + 1, J1, 1},
             member_opt(m, GemmOpt(), m.sA, m.sA, m.sA));
    return j + 1;
}

// Record event (kind, i) on stream `from` and make every stream of `to` wait for it: the fork, every join and the hand-over
// of a finished panel.  (A null entry is a stream that takes no part this time.)
static void record_wait(gp_ctx *g, int kind, size_t i, hipStream_t from, std::initializer_list<hipStream_t> to) {
    hipEvent_t e = la_event(g, kind, i);
    GP_NOTE(hipEventRecord(e, from));
    for (hipStream_t t : to)
        if (t) GP_NOTE(hipStreamWaitEvent(t, e, 0));
}

// C[r0 .. R1, c0 .. c1) -= A[:, J0 .. J1) A[c0 .. c1, J0 .. J1)^T of m.A on stream s: the update every tile right of a panel takes from it
static void panel_update(gp_ctx *g, hipStream_t s, const Members &m, int J0, int J1, TileSet ts) {
    const double *P = m.A + (long)J0 * GP_TILE;
    gemm(g, s, 1, m.A, m.lda, P, m.lda, P, m.lda, 1, (J1 - J0) * GP_TILE, ts, member_opt(m, GemmOpt(), m.sA, m.sA, m.sA));
}

void factor_buf(gp_ctx *g, const Members &m, int nt, int R1, bool side_inv) {
    const int W = g->panel_tiles;
    hipStream_t s = g->s;
    if (side_inv) record_wait(g, EV_MISC, 0, s, {g->s_inv});
    for (int J0 = 0; J0 < nt; J0 += W) {
        const int J1 = std::min(J0 + W, nt);
        for (int j = J0; j < J1;) j = chain_step(g, s, m, j, J1, R1);
        if (side_inv) {
            record_wait(g, EV_CHAIN, J0 / W, s, {g->s_inv});
            build_panel_inv_one(g, g->s_inv, J0 / W, W, nt);
        }
        // trailing update with the whole panel (K = W * 128): the dense contraction on MFMA
        if (J1 < nt) panel_update(g, s, m, J0, J1, TileSet{0, R1, J1, nt, 1});
    }
    if (side_inv) record_wait(g, EV_MISC, 4, g->s_inv, {s});
}

// The single-stream factorisation of the model's Ky (N <= 768, and the sizes where the look-ahead's per-panel events, waits and
// separate look-ahead launch cost more than the overlap gives: measured 1.99 vs 2.31 ms at N = 4096, 0.84 vs 1.05 at N = 2048,
// equal from N = 5120 on; same arithmetic, bitwise the same factor).  Panels wider than the matrix take the batched inverse build.
int factor(gp_ctx *g) {
    const int nt = (int)(g->Npad / GP_TILE);
    const int W = g->panel_tiles;
    const bool side = nt > W && g->s_inv;
    int rc;
    if (side && (rc = reserve_panel_inv(g, W, nt))) return rc;
    factor_buf(g, ctx_members(g), nt, nt + 1, side);
    if (side) {
        g->invp_W = W;
        g->invp_valid = true;   // (fit_impl drops it again when the attempt turns out not positive definite)
        return la_events_ok(g);
    }
    return 0;
}

// ---- the look-ahead scheduler: factor_lookahead's panel loop over the strands below ----
// What one factorisation is laid out as, computed once before the loop (host arithmetic only).
struct LaPlan {
    int nt, R1, W, nJ;
    std::vector<int> pb;      // panel boundaries (uniform panels of W tiles; two sentinels)
    int pstages, pred_start;  // pipelined stages: how many ride behind the factorisation, and the panel that releases them
    bool emu;                 // the trailing update runs in residue form
    int Gf;                   // emulated: panels per residue launch (the far launches ride on the otherwise idle candidate stream)
    int edge(int k) const { return pb[std::min(k, nJ + 1)]; }
};
static LaPlan la_plan(const gp_ctx *g, const PredPipe &pp) {
    LaPlan p;
    p.nt = (int)(g->Npad / GP_TILE);
    p.R1 = p.nt + 1;
    p.W = g->panel_tiles;
    for (int j = 0; j < p.nt; j += p.W) p.pb.push_back(j);
    p.pb.push_back(p.nt);
    p.pb.push_back(p.nt);
    p.nJ = (int)p.pb.size() - 2;
    // Only the first `pipe_stages` candidate stages ride behind the factorisation (on the CU-masked stream, released
    // at panel pred_start); the caller runs the rest on the main stream, on every CU, once the factor is complete.
    p.pstages = pp.on ? std::max(1, std::min(p.nJ, pp.stages)) : 0;
    p.pred_start = std::max(0, std::min(p.nJ - 1, p.nJ * pp.start_pct / 100));
    p.emu = emu_fit_applies(g);
    p.Gf = (p.emu && !pp.on) ? std::max(1, std::min(g->rns_group_fit, (int)(GP_RNS_KMAX / ((long)p.W * GP_TILE)))) : 1;
    return p;
}

// Columns owned by the chain stream (options own_keep_*): in the head of the factorisation the chain finishes panel J+1 long
// before bulk(J) has drained and would wait for it, with the CUs kept free of the bulk stream idle.  bulk(J) therefore keeps
// only what lasts as long as the chain is busy with the next panel (a count of tiles linear in the rows below it); the
// rest -- the last tile columns oc .. nt -- takes panel J's update on THIS stream, after chain(J), on every CU.  The owned
// range only shrinks with J, so own(J) never meets a tile bulk(J-1) writes, and a column handed back to the bulk stream
// had its last update here before chain(J+1), which bulk(J+1) waits for.  Same contraction per tile in the same order:
// the same bits as without.
// Returns oc for the panel whose look-ahead target ends at tile J2; own_prev is the count owned at the previous panel (nt before the first).
static int first_owned_column(int nt, int J2, int W, int own_prev, int keep_base, int keep_per_row, int keep_pipe_pct, bool piped) {
    if (keep_per_row <= 0 || J2 >= nt) return nt;
    const long n = nt - J2;
    // tiles right of J2 (with the rhs row) minus the kept ones (the chain's time per panel grows with the panel width: per_row is per 6 tiles)
    long keep = keep_base + (long)keep_per_row * n * W / 6;
    // (one-call entry points: once the candidate stages share the bulk stream's CUs the trailing update lasts longer and the
    // chain waits again; the bulk stream then keeps own_keep_pipe_pct % of the rule's share)
    // (never at the FIRST panel that owns columns: there own_prev is still its initial nt, and keep = 0 would hand the
    // whole trailing update to the chain stream -- pipe_start_pct = 0, or so few panels that pred_start rounds to 0)
    if (piped && own_prev < nt) keep = keep * keep_pipe_pct / 100;
    const long t_own = n * (n + 1) / 2 + n - keep;
    int c = 0;
    while (c < own_prev && (long)(c + 1) * (c + 2) / 2 + (c + 1) <= t_own) ++c;
    return nt - c;
}

// Two concurrent MFMA-bound launches run slower than one after the other (measured 51 vs 63 TFLOP/s), and
// the candidate stream is CU-masked like the trailing update (the diagonal-tile workgroup needs an empty
// CU), which costs it 1/8 of the chip.  So only the first `pipe_stages` stages ride here, released once
// the factorisation turns latency-bound (panel >= pred_start): they fill the CUs the chain leaves idle in
// the tail.  The rest run after the join on the main stream, on every CU (fit_impl).  Measured at C3:
// 73.4 ms against 77.0 for gp_fit + gp_predict; every stage pipelined: 78.1.
// Releases the stages that panel J (>= pred_start) makes runnable; m is the context's members with the width in use (T / T2 are the pipe's T / S).
static void release_stages(gp_ctx *g, const LaPlan &p, const PredPipe &pp, const Members &m, int J, int *next) {
    for (; *next <= J && *next < p.pstages; ++*next) {
        const int Q = *next;
        GP_NOTE(hipStreamWaitEvent(g->s_pred, la_event(g, EV_CHAIN, J), 0));
        GP_NOTE(hipStreamWaitEvent(g->s_pred, la_event(g, EV_INVP, Q), 0));
        solve_step(g, g->s_pred, m, Q, pp.trapezoid ? std::min(pp.mt, p.edge(Q + 1)) : pp.mt);
    }
}

// fp64 trailing update of panel J on the bulk stream: everything between the look-ahead target and the owned columns
static void trail_fp64(gp_ctx *g, const LaPlan &p, const Members &m, int J, int oc) {
    if (p.pb[J + 2] < oc) panel_update(g, g->s_bulk, m, p.pb[J], p.pb[J + 1], TileSet{0, p.R1, p.pb[J + 2], oc, 1});
    GP_NOTE(hipEventRecord(la_event(g, EV_BULK, J), g->s_bulk));
}

// "emulate_fp64": the trailing update (the launches of the bulk stream) in residue form on the int8 matrix cores
// (rns.hip).  The Schur complement right of the look-ahead panel lives as Ky (untouched, in dA) minus an exact integer
// accumulator dRm; a panel's columns are rebuilt in fp64 once, right before they become the look-ahead target.  The
// chain (diagonal tiles, panel solves, in-panel and look-ahead updates) and the right-hand-side tile row stay fp64.
//
// Panels in groups of Gf (all panel edges sit on 256-column accumulator blocks).  Pair (panel j, column
// panel c >= j+2; c = j+1 is the fp64 look-ahead) is served exactly once, by
//   near(J)  on the bulk stream, every iteration: the group's panels so far -> the columns of panel J+2,
//   mid(g)   on the bulk stream, from the group's last panel on, ONE column panel per iteration: the whole group
//            -> the next Gf column panels, each slice an iteration before its columns are rebuilt (as one
//            launch of 3.7 ms at N = 16384 it sat in front of near(J+1) and the chain stalled 2.6 ms behind it),
//   far(g)   on a stream of its own: the whole group -> everything right of that,
// so the accumulator makes one round trip per group for the far columns and the long launch (K = Gf PB)
// overlaps the next group's chain.  Ordering: near(J) and mid(g) accumulate into blocks far(g-1) / far(g-2)
// wrote (mid waits for far(g-1); near follows mid(g-1) in stream order); far(g) follows far(g-1) in stream
// order; the chain's reconstruction of panel J+1's columns waits for bulk(J-1) = near(J-1), recorded
// BEFORE mid so that the chain does not wait for it.  The integers summed are those of Gf = 1.
struct EmuTrail {
    gp_ctx *g;
    const LaPlan &p;
    const Members &m;
    RnsGeom rg;
    std::vector<char> far_issued;
    int mid_Jg = -1, mid_end = 0, mid_first = 0, mid_base = 0, mid_next = 0;   // the slices of mid(g) still to come

    int prepare() {
        int rc;
        if ((rc = rns_prepare(g, g->jitter_try, &rg))) return rc;
        far_issued.assign(p.nJ / p.Gf + 2, 0);
        return g->dRm.reserve((long)GP_RNS_T * rg.nt256 * rg.nt256 * 65536);
    }
    // panels Jfirst .. (tiles up to Tend) -> tile columns [t0, t1)
    void rlaunch(hipStream_t st, int Jfirst, int Tend, int t0, int t1, int first) const {
        t1 = std::min(t1, p.nt);
        if (t0 >= t1) return;
        const int T0 = p.pb[Jfirst];
        rns_gemm(g, st, g->dLr + (long)T0 * GP_TILE, rg.Lpitch, rg.Lplane, g->dLr + (long)T0 * GP_TILE, rg.Lpitch, rg.Lplane,
                 g->dRm, rg.nt256, rg.nt256, rg.nt256, t0 / 2, (t1 + 1) / 2, (Tend - T0) * GP_TILE, first, 1);
    }
    // rebuild the columns of panel J+2 in fp64 (Ky minus everything accumulated for them: panels 0 .. J) as soon as
    // the last residue launch into them is enqueued -- on this stream, off the chain
    void rebuild_next(int J) const {
        if (p.edge(J + 2) < p.nt)
            launch_rns_reconstruct256(g->s_bulk, g->dRm, rg.nt256, rg.nt256, rg.nt256, p.edge(J + 2), std::min(p.edge(J + 3), p.nt),
                                      g->Npad, m.A, m.lda, rg.back, 1);
    }
    // panel J's share, on the bulk stream (and the far stream): records bulk(J)
    void update(int J) {
        hipStream_t sb = g->s_bulk, sfar = g->s_pred;
        const int J1 = p.pb[J + 1], J2 = p.pb[J + 2], Gf = p.Gf;
        rns_convert_panel(g, sb, rg, J, g->dInfo + 2);
        // the right-hand-side tile row rides in fp64
        panel_update(g, sb, m, p.pb[J], J1, TileSet{p.nt, p.R1, J2, p.nt, 0});
        if (Gf == 1) {
            rlaunch(sb, J, J1, J2, p.nt, J == 0 ? 1 : 0);
            rebuild_next(J);
            GP_NOTE(hipEventRecord(la_event(g, EV_BULK, J), sb));
            return;
        }
        const int gi = J / Gf, Jg = gi * Gf;
        const int first = gi == 0 ? 1 : 0;
        GP_NOTE(hipEventRecord(la_event(g, EV_CONV, J), sb));
        rlaunch(sb, Jg, J1, p.edge(J + 2), p.edge(J + 3), first);
        rebuild_next(J);
        GP_NOTE(hipEventRecord(la_event(g, EV_BULK, J), sb));
        if (J % Gf == Gf - 1) {
            if (gi >= 1 && far_issued[gi - 1]) GP_NOTE(hipStreamWaitEvent(sb, la_event(g, EV_FAR, gi - 1), 0));
            mid_Jg = Jg;            // the slices of mid(g): column panel mid_base + k at iteration J + k
            mid_end = J1;
            mid_first = first;
            mid_base = J + 3;
            mid_next = 0;
            if (p.edge(J + 3 + Gf) < p.nt) {
                GP_NOTE(hipStreamWaitEvent(sfar, la_event(g, EV_CONV, J), 0));
                rlaunch(sfar, Jg, J1, p.edge(J + 3 + Gf), p.nt, first);
                GP_NOTE(hipEventRecord(la_event(g, EV_FAR, gi), sfar));
                far_issued[gi] = true;
            }
        }
        if (mid_Jg >= 0 && mid_next < Gf) {
            rlaunch(sb, mid_Jg, mid_end, p.edge(mid_base + mid_next), p.edge(mid_base + mid_next + 1), mid_first);
            ++mid_next;
        }
    }
};

int factor_lookahead(gp_ctx *g, const PredPipe &pp) {
    int rc;
    if ((rc = ensure_bulk_stream(g))) return rc;
    const LaPlan p = la_plan(g, pp);
    const int nt = p.nt;
    hipStream_t sp = g->s_panel, sb = g->s_bulk;
    // the candidate stream takes part for the pipelined stages or, emulated, for the far launches (never both: Gf > 1 only without a pipe)
    hipStream_t spred = pp.on ? g->s_pred : nullptr, sfar = p.Gf > 1 ? g->s_pred : nullptr;
    // Every inverted diagonal panel (alpha, the candidate solve and Ky^-1 all need them) is built on the side stream as soon
    // as its panel of L is final, beside the rest of the factorisation: after the join nothing is left to build (as a pass of
    // its own, 2W - 1 short launches in series, it held the main stream for 0.3 ms between the factor and its first consumer).
    if ((rc = reserve_panel_inv(g, p.W, nt))) return rc;
    Members cm = ctx_members(g);
    cm.W = p.W;   // (g->invp_W is set at the end only: the pipelined stages, which run on cm.T / cm.T2, need the width now)
    // fork
    record_wait(g, EV_MISC, 0, g->s, {sp, sb, g->s_inv, spred, sfar});
    if (pp.on && pp.init) pp.init(spred);
    EmuTrail emu{g, p, cm};
    if (p.emu && (rc = emu.prepare())) return rc;
    int next_pred = 0;
    int own_prev = nt;   // columns owned by the chain stream at the previous panel (the range never grows)
    for (int J = 0; J < p.nJ; ++J) {
        const int J0 = p.pb[J], J1 = p.pb[J + 1], J2 = p.pb[J + 2];
        for (int j = J0; j < J1;) j = chain_step(g, sp, cm, j, J1, p.R1);
        record_wait(g, EV_CHAIN, J, sp, {g->s_inv});
        build_panel_inv_one(g, g->s_inv, J, p.W, nt);
        if (J < p.pstages) GP_NOTE(hipEventRecord(la_event(g, EV_INVP, J), g->s_inv));
        if (pp.on && J >= p.pred_start) release_stages(g, p, pp, cm, J, &next_pred);
        if (J1 >= nt) break;
        const int oc = p.emu ? nt : first_owned_column(nt, J2, p.W, own_prev, g->own_keep_base, g->own_keep_per_row,
                                                       g->own_keep_pipe_pct, pp.on && J >= p.pred_start);
        own_prev = nt - oc;
        if (oc < nt && J >= 1) panel_update(g, sp, cm, J0, J1, TileSet{0, p.R1, oc, nt, 1});
        // the look-ahead update is on the critical path: enqueue it before the trailing update so that its
        // workgroups reach the dispatcher first once bulk(J-1) has drained
        if (J >= 1) GP_NOTE(hipStreamWaitEvent(sp, la_event(g, EV_BULK, J - 1), 0));
        // (emulated: the look-ahead panel's columns took everything the residue accumulator holds for them -- panels
        // 0 .. J-1 -- on the bulk stream, before bulk(J-1) was recorded)
        panel_update(g, sp, cm, J0, J1, TileSet{0, p.R1, J1, J2, 1});
        if (oc < nt && J == 0)   // (the first panel has no bulk launch to wait for: the critical update goes first)
            panel_update(g, sp, cm, J0, J1, TileSet{0, p.R1, oc, nt, 1});
        if (J2 >= nt) continue;
        GP_NOTE(hipStreamWaitEvent(sb, la_event(g, EV_CHAIN, J), 0));
        if (p.emu) emu.update(J);
        else trail_fp64(g, p, cm, J, oc);
    }
    // join  (every far launch ends before the factor is complete: mid of the next group waits for it; join anyway)
    record_wait(g, EV_MISC, 1, sp, {g->s});
    record_wait(g, EV_MISC, 2, sb, {g->s});
    if (sfar) record_wait(g, EV_MISC, 7, sfar, {g->s});
    g->pipe_done = p.pstages;
    if (spred) record_wait(g, EV_MISC, 3, spred, {g->s});
    record_wait(g, EV_MISC, 4, g->s_inv, {g->s});
    g->invp_W = p.W;
    g->invp_valid = true;   // (fit_impl drops it again when the attempt turns out not positive definite)
    return la_events_ok(g);   // (an error return makes fit_impl quiesce every stream before it reports)
}

__device__ __forceinline__ void dot_ay_body(const double *alpha, long lda_, const double *Y, long N, int P, double *out) {
    __shared__ double sh[16];
    const int p = blockIdx.x;
    double s = 0.0;
    for (long i = threadIdx.x; i < N; i += 1024) s = fma(alpha[p * lda_ + i], Y[i * P + p], s);
    // block reduce
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = 0.0;
        for (int i = 0; i < 16; ++i) r += sh[i];
        out[p] = r;
    }
}

__global__ void dot_ay_kernel(const double *alpha, long lda_, const double *Y, long N, int P, double *out) {
    dot_ay_body(alpha, lda_, Y, N, P, out);
}
// member z = blockIdx.z of gp_fit_grad_batch: alpha + z sV, targets Y + z sY (0: shared), results at out + z so
__global__ void dot_ay_batch_kernel(const double *alpha, long sV, long lda_, const double *Y, long sY, long N, int P, double *out,
                                    long so) {
    const long z = blockIdx.z;
    dot_ay_body(alpha + z * sV, lda_, Y + z * sY, N, P, out + z * so);
}
static void launch_dot_ay(hipStream_t s, const double *alpha, long lda_, const double *Y, long N, int P, double *out, int nb, long sV,
                          long so, long sY) {
    if (nb > 1)
        GP_LAUNCH(dot_ay_batch_kernel, dim3(P, 1, nb), dim3(1024), 0, s, alpha, sV, lda_, Y, sY, N, P, out, so);
    else
        GP_LAUNCH(dot_ay_kernel, dim3(P), dim3(1024), 0, s, alpha, lda_, Y, N, P, out);
}

// log det, alpha = L^-T z and alpha . y of m's members: 45 short dependent launches
void alpha_lml(gp_ctx *g, hipStream_t s, const Members &m) {
    const long Npad = g->Npad;
    launch_logdet(s, m.A, m.lda, g->N, m.scal + SCAL_LOGDET.off, m.nb, m.sA, m.sS);
    launch_trsv_backward(s, m.A, m.lda, m.invP, m.W, Npad, m.A + Npad * m.lda, m.lda, g->P, m.alpha, m.w, m.nb, m.sA, m.sP, m.sV);
    launch_dot_ay(s, m.alpha, Npad, m.Y, g->N, g->P, m.scal + SCAL_DOT.off, m.nb, m.sV, m.sS, m.sY);
}

// ---- host arithmetic of one fit, per member ----
// what the diagonal of K gets, and the diagonal of Ky the jitter ladder starts from
void ky_diag(const KernParams &kp, double noise, double *diag_add, double *diag0) {
    *diag_add = noise + 1e-8;  // exact_gaussian_inference.py:56
    *diag0 = (kp.gower ? std::pow(kp.variance, kp.D) : kp.variance) + *diag_add;
}
// One step of the jitter ladder (GPy/GPy/util/linalg.py:62-75) after an attempt that failed with `info`: 0 with the next jitter
// in *jitter, or the code the fit ends with.
int ladder_step(double diag0, int maxtries, int info, double *jitter, int *tries) {
    if (!(diag0 > 0.0)) return GP_ERR_NOT_PD_DIAG;
    *jitter = *tries == 0 ? diag0 * 1e-6 : *jitter * 10.0;
    ++*tries;
    if (*tries > maxtries || !std::isfinite(*jitter)) return info > 0 ? info : 1;
    return 0;
}
int ladder_failure(int st) {
    if (st == GP_ERR_NOT_PD_DIAG) return fail(st, "not pd: non-positive diagonal elements");
    if (st) g_err = "not positive definite, even with jitter.";
    return st;
}
// the ladder per member (api_internal.h): runs of consecutive failed members share launches
int members_ladder(gp_ctx *g, const Members &m, int nt, int maxtries, std::vector<int> &active, std::vector<double> &jit, double *dJit,
                   std::vector<int> &st, const MembersBuild &build, const MembersDiag0 &diag0) {
    const int R = m.nb;
    std::vector<int> tries(R, 0), info(4 * (size_t)R);
    std::vector<double> d0(R, 0.0);
    for (int round = 0;; ++round) {
        if (round > 0 && dJit) HIPCHK(hipMemcpyAsync(dJit, jit.data(), sizeof(double) * R, hipMemcpyHostToDevice, g->s));
        for (int m0 = 0, m1; m0 < R; m0 = m1 + 1) {   // [m0, m1): a run of consecutive active members
            for (m1 = m0; m1 < R && active[m1];) ++m1;
            if (m1 == m0) continue;
            const Members run = members_range(m, m0, m1 - m0);
            if (int rc = build(run, m0, round > 0)) return rc;
            HIPCHK(hipMemsetAsync(run.info, 0, sizeof(int) * 4 * run.nb, g->s));
            factor_buf(g, run, nt, nt + 1);
        }
        HIPCHK(hipMemcpyAsync(info.data(), m.info, sizeof(int) * 4 * R, hipMemcpyDeviceToHost, g->s));
        GP_SYNC(g->s);
        if (round == 0) {
            std::vector<int> failed;
            for (int r = 0; r < R; ++r)
                if (active[r] && info[4 * r] != 0) failed.push_back(r);
            if (int rc = failed.empty() ? 0 : diag0(failed, d0)) return rc;
        }
        bool again = false;
        for (int r = 0; r < R; ++r) {
            if (!active[r]) continue;
            if (info[4 * r] != 0) st[r] = ladder_step(d0[r], maxtries, info[4 * r], &jit[r], &tries[r]);
            active[r] = info[4 * r] != 0 && st[r] == 0;
            again = again || active[r];
        }
        if (!again) return 0;
    }
}
// the exact model's: every member of m, Ky by build_ky (which adds the jitter and sets the RHS rows), diag0 from ky_diag
int ky_ladder(gp_ctx *g, const Members &m, int maxtries, const std::vector<double> &diag0, std::vector<double> &jit, double *dJit,
              std::vector<int> &st) {
    std::vector<int> active(m.nb, 1);
    return members_ladder(g, m, (int)(g->Npad / GP_TILE), maxtries, active, jit, dJit, st,
                          [&](const Members &run, int, bool jittered) {
                              build_ky(g, run, jittered);
                              return 0;
                          },
                          [&](const std::vector<int> &failed, std::vector<double> &d0) {
                              for (int r : failed) d0[r] = diag0[r];
                              return 0;
                          });
}
// scal: [0] log det, [8, 8 + P) alpha . y
double lml_from_scalars(long N, int P, const double *scal) {
    double fit = 0.0;
    for (int p = 0; p < P; ++p) fit += scal[SCAL_DOT.off + p];
    const double log_2_pi = std::log(2.0 * M_PI);
    return 0.5 * (-(double)N * P * log_2_pi - P * scal[SCAL_LOGDET.off] - fit);  // exact_gaussian_inference.py:62
}

// The factorisation's status word, read back (the stream is drained); *bad, when `emu`: an entry of L left the fixed-point range
// of the residue path.
int factor_status(gp_ctx *g, bool emu, int *info, int *bad) {
    *bad = 0;
    HIPCHK(hipMemcpyAsync(info, g->dInfo, sizeof(int), hipMemcpyDeviceToHost, g->s));
    GP_SYNC(g->s);
    if (emu && *info == 0) HIPCHK(hipMemcpy(bad, g->dInfo + 2, sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

// Any error return of fit_impl after work was forked onto the side streams must leave them joined: the guard waits for
// every stream of the context unless the normal exit (where the joins are stream-ordered) dismissed it.
struct QuiesceOnError {
    gp_ctx *g;
    bool armed = true;
    ~QuiesceOnError() {
        if (!armed) return;
        for (hipStream_t st : {g->s_panel, g->s_bulk, g->s_inv, g->s_pred, g->s})
            if (st) hipStreamSynchronize(st);
    }
};

// The PredPipe of a kind: buffers, what fills T, and how many stages ride behind the factorisation from which panel on.
static int make_pipe(gp_ctx *g, Pipe kind, PredPipe *pp) {
    const long N = g->N, Npad = g->Npad;
    const int nt = (int)(Npad / GP_TILE), W = std::min(g->panel_tiles, nt), nJ = (nt + W - 1) / W;
    const bool cand = kind == Pipe::Candidates;
    const long mcpad = cand ? round_up(g->M, GP_TILE) : Npad;
    int rc;
    if (cand && (rc = ensure_out(g))) return rc;
    if ((rc = g->dT.reserve(mcpad * Npad))) return rc;
    if ((rc = g->dT2.reserve(mcpad * Npad))) return rc;
    if (!cand && (rc = g->dWi.reserve(Npad * Npad))) return rc;
    if ((rc = reserve_panel_inv(g, W, nt))) return rc;
    pp->on = true;
    pp->mt = (int)(mcpad / GP_TILE);
    pp->nJ = nJ;
    pp->trapezoid = !cand;
    // stages and release point; 0 / -1 = automatic: the share of the panels that was best at N = 16384 (3 of 22 candidate
    // stages, 8 of 22 L^-T stages), released at 32 % of up to 24 panels, 40 % beyond (measured N = 8192 ... 32768)
    if (cand) {
        pp->init = [g, mcpad, N, Npad](hipStream_t st) { launch_cross_k(st, g->dT, Npad, g->dXs, g->M, mcpad, g->dX, N, Npad, g->kp); };
        pp->phase = "cholesky+cand_solve";
        pp->rest_phase = "cand_solve_rest";
        pp->flops = (double)N * N * N / 3.0 + (double)N * N * g->M;
        pp->stages = g->pipe_stages;
        if (pp->stages <= 0) pp->stages = std::max(1, (nJ * 14 + 50) / 100) + (nJ <= 12 ? 1 : 0);   // small N: the chain is everything
        pp->start_pct = g->pipe_start_pct;
        if (pp->start_pct < 0) pp->start_pct = nJ <= 24 ? 32 : 40;
    } else {
        pp->init = [g, Npad](hipStream_t st) { launch_set_identity(st, g->dT, Npad, Npad); };
        pp->phase = "cholesky+potri_stages";
        pp->rest_phase = "potri_solve_rest";
        pp->flops = (double)N * N * N / 3.0;
        pp->stages = g->pipe_stages_grad;
        if (pp->stages <= 0) pp->stages = std::max(1, (nJ * 36 + 50) / 100);
        pp->start_pct = g->pipe_start_pct_grad;
    }
    return 0;
}

// One attempt of the ladder, as two phases: Ky with this jitter, then its factor -- pipelined, look-ahead or single-stream.
static int factor_attempt(gp_ctx *g, const PredPipe &pp, const double *diag_add, const double *jitter) {
    const double N = (double)g->N;
    const int nt = (int)(g->Npad / GP_TILE);
    g->lr_valid = false;     // residue planes of L belong to one factorisation attempt
    g->jitter_try = *jitter;
    int ph = phase_begin(g, "kbuild", 0.0, 8.0 * N * g->D + 8.0 * N * N / 2);
    Members m = ctx_members(g);
    m.diag = diag_add;
    m.jit = jitter;
    build_ky(g, m, *jitter != 0.0);
    phase_end(g, ph);
    HIPCHK(hipMemsetAsync(g->dInfo, 0, sizeof(int) * 4, g->s));
    ph = phase_begin(g, pp.on ? pp.phase : "cholesky", pp.on ? pp.flops : N * N * N / 3.0, 0.0);
    // (the emulated trailing update lives in the look-ahead scheduler)
    const bool la = pp.on || (g->lookahead && nt > g->panel_tiles && (nt > g->lookahead_min_tiles || emu_fit_applies(g)));
    const int rc = la ? factor_lookahead(g, pp) : factor(g);
    if (rc) return rc;
    phase_end(g, ph);
    return 0;
}

// The stages the pipe left to do, on the main stream and every CU.  alpha = L^-T z, log det and alpha'y are 45 short dependent
// launches (latency-bound, 1 ms): while stages are still to run they go on the side stream, beside those long launches
// (*side_alpha: done there, EV_MISC 6 marks their end).
static int rest_stages(gp_ctx *g, const PredPipe &pp, bool *side_alpha) {
    if (g->pipe_done >= pp.nJ) return 0;
    const int phr = phase_begin(g, pp.rest_phase, 0.0, 0.0);
    const int rci = ensure_panel_inv(g);
    if (rci) return rci;
    *side_alpha = g->s_inv && g->side_alpha;
    hipEvent_t eI = la_event(g, EV_MISC, 5);
    if (*side_alpha) GP_NOTE(hipEventRecord(eI, g->s));
    // the long launches first: the 45 short launches of alpha / log det take the host 0.7 ms to enqueue, during which
    // the main stream sat empty when they went first
    solve_rows(g, ctx_members(g), pp.mt, pp.trapezoid, g->pipe_done);
    if (*side_alpha) {
        GP_NOTE(hipStreamWaitEvent(g->s_inv, eI, 0));
        alpha_lml(g, g->s_inv, ctx_members(g));
        GP_NOTE(hipEventRecord(la_event(g, EV_MISC, 6), g->s_inv));
    }
    phase_end(g, phr);
    return 0;
}

// Shared body of gp_fit, gp_fit_predict and gp_fit_grad.  With a pipe the solve of the resident candidates (or of the identity,
// for Ky^-1) is pipelined behind the factorisation (PredPipe) and finished afterwards; Candidates appends the posterior reductions.
int fit_impl(gp_ctx *g, int maxtries, Pipe kind, int include_noise) {
    HIPCHK(hipSetDevice(g->device));
    QuiesceOnError guard{g};
    const long N = g->N, Npad = g->Npad;
    const int P = g->P;
    int rc;
    if (g->lap.on) fit_dropped(g);   // a Laplace-fitted context: its factor goes, and gp_set_params' noise is back before ky_diag reads it
    if ((rc = mean_residuals(g))) return rc;   // a resident mean function: dY = Y - m(X) is what everything below factors against
    PredPipe pp;
    if (kind != Pipe::None && (rc = make_pipe(g, kind, &pp))) return rc;
    double diag_add, diag0;
    ky_diag(g->kp, g->noise, &diag_add, &diag0);
    g->nphases = 0;
    g->emu_off_call = false;
    fit_dropped(g);

    // the jitter ladder, GPy/GPy/util/linalg.py:62-75
    double jitter = 0.0;
    int tries = 0;  // number of jittered attempts so far
    for (int info = 0, bad = 0;;) {
        if ((rc = factor_attempt(g, pp, &diag_add, &jitter))) return rc;
        if ((rc = factor_status(g, g->emulate_fp64 && !g->emu_off_call, &info, &bad))) return rc;
        if (bad) {
            // emulation fallback -- an entry of L outside the fixed-point range (non-finite data): the same attempt again in
            // true fp64, whose result is what the reference would return for such data
            g->emu_off_call = true;
            ++g->emu_fallbacks;
            g->nphases = 0;
            g->invp_valid = false;
            continue;
        }
        if (info == 0) break;
        g->invp_valid = false;
        const int rcl = ladder_step(diag0, maxtries, info, &jitter, &tries);
        if (rcl == GP_ERR_NOT_PD_DIAG) return fail(rcl, "not pd: non-positive diagonal elements");
        if (rcl) {
            g_err = "not positive definite, even with jitter.";
            return rcl;
        }
        g->nphases = 0;
    }
    g->jitter = jitter;

    // what the pipe left over, with alpha on the side stream where that pays; Ky^-1 from the identity's solve
    bool side_alpha = false;
    if (pp.on && (rc = rest_stages(g, pp, &side_alpha))) return rc;
    if (kind == Pipe::Identity) {
        if ((rc = wi_lauum(g))) return rc;
        g->wi_valid = true;
        g->w_in_t2 = true;   // dT2 = L^-T of this factor: ensure_linv transposes it instead of solving again
    }
    int ph = phase_begin(g, "alpha_lml", 2.0 * (double)N * N * P, 8.0 * (double)N * N / 2);
    if (side_alpha) {
        GP_NOTE(hipStreamWaitEvent(g->s, la_event(g, EV_MISC, 6), 0));
    } else {
        if ((rc = ensure_panel_inv(g))) return rc;
        alpha_lml(g, g->s, ctx_members(g));
    }
    phase_end(g, ph);
    if (kind == Pipe::Candidates) {
        ph = phase_begin(g, "reduce", 0.0, 8.0 * (double)N * g->M);
        launch_predict_reduce(g->s, g->dT2, Npad, g->M, N, g->dA + Npad * Npad, Npad, P, g->kp.variance,
                              include_noise ? g->noise : 0.0, g->dMean, g->dVar);
        mean_add(g, g->dXs, g->M, g->dMean);
        phase_end(g, ph);
    }

    // read-back
    std::vector<double> sc(SCAL_DOT.off + P);   // log det ... the last output's alpha . y
    HIPCHK(hipMemcpyAsync(sc.data(), g->dScal, sizeof(double) * sc.size(), hipMemcpyDeviceToHost, g->s));
    GP_SYNC(g->s);
    g->logdet = sc[SCAL_LOGDET.off];
    g->lml = lml_from_scalars(N, P, sc.data());
    g->fitted = true;
    if (kind == Pipe::Candidates) {
        g->predicted = true;
        g->predicted_noise = include_noise ? 1 : 0;
    }
    guard.armed = false;
    return 0;
}

extern "C" int gp_fit(gp_t *g, int maxtries, double *lml, double *logdet, double *jitter_used) {
    if (!g) return fail(GP_ERR_ARG, "null gp");
    GP_DEAD_CHECK(g);
    if (!g->have_data || !g->have_params) return fail(GP_ERR_STATE, "set data and params before gp_fit");
    int rc = fit_impl(g, maxtries, Pipe::None, 0);
    if (rc) return rc;
    if (lml) *lml = g->lml;
    if (logdet) *logdet = g->logdet;
    if (jitter_used) *jitter_used = g->jitter;
    return 0;
}

// gp_fit followed by gp_predict on the resident candidates, as ONE pipelined pass (the BO loop always runs
// them back to back: GPyOpt/GPyOpt/core/bo.py:236-254 then acquisitions/base.py:33-39).  Results are those of
// the two separate calls; the candidate solve merely overlaps the factorisation's latency-bound phases.
extern "C" int gp_fit_predict(gp_t *g, int maxtries, int include_noise, double *lml, double *logdet, double *jitter_used,
                   double *mean, double *var) {
    if (!g) return fail(GP_ERR_ARG, "null gp");
    GP_DEAD_CHECK(g);
    if (!g->have_data || !g->have_params) return fail(GP_ERR_STATE, "set data and params before gp_fit_predict");
    if (g->M < 1) return fail(GP_ERR_STATE, "gp_set_candidates first");
    HIPCHK(hipSetDevice(g->device));
    const int nt = (int)(g->Npad / GP_TILE);
    // the emulated candidate solve runs after the factorisation (its residue planes of L need the complete factor)
    // (a handful of candidates take the matrix-vector solve of gp_predict after the factorisation: both entry points then
    // return the same bits)
    const bool can_pipe = g->lookahead && nt > g->panel_tiles && round_up(g->M, GP_TILE) <= g->mc_max && !g->emulate_fp64 &&
                          g->M > g->small_m;
    int rc;
    if (can_pipe) {
        if ((rc = fit_impl(g, maxtries, Pipe::Candidates, include_noise))) return rc;
    } else {
        if ((rc = fit_impl(g, maxtries, Pipe::None, 0))) return rc;
        if ((rc = ensure_out(g))) return rc;
        if ((rc = run_predict(g, include_noise))) return rc;
    }
    if (lml) *lml = g->lml;
    if (logdet) *logdet = g->logdet;
    if (jitter_used) *jitter_used = g->jitter;
    if (mean) HIPCHK(hipMemcpyAsync(mean, g->dMean, sizeof(double) * g->M * g->P, hipMemcpyDeviceToHost, g->s));
    if (var) HIPCHK(hipMemcpyAsync(var, g->dVar, sizeof(double) * g->M, hipMemcpyDeviceToHost, g->s));
    GP_SYNC(g->s);
    return 0;
}
