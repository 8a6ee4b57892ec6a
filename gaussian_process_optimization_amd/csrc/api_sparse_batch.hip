// gp_sparse_fit_grad_batch: the sparse model's LML and its gradients for R (Z, variance, lengthscale, noise) members over the
// context's (X, Y) in one call -- the L-BFGS evaluations of R hyper-parameter restarts of GPModel(sparse=True) in lockstep
// (SparseGPRegression.optimize_restarts(parallel=True)).  Reference per member: VarDTC.inference and SparseGP._update_gradients as
// listed in api_sparse.hip; the restarts: GPModel.updateModel (GPyOpt/GPyOpt/models/gpmodel.py:78-93).
//
// The launch sequence is gp_sparse_fit_grad's (sparse_fit_impl + its gradient half, api_sparse.hip) with the member as a batch
// index of every launch: blockIdx.z / .y of the K-build, the cross covariance, the tile Cholesky, the helpers and the gradient
// pass of sparse.hip, the batch dimension of the GEMM.  A launch over members runs the body of the single call's kernel, and
// gemm() takes the instance it picks for ONE member's tiles: a member does the single call's arithmetic, bit for bit, whatever R,
// its slot and its company.  woodbury_inv, which no output of this call depends on, is not formed.
// Both jitter ladders (Kmm, then B) are members_ladder (api_internal.h), the one the exact batch and the ensemble run: a failed
// member is factored again with the next jitter, alone with the other failed members -- runs of consecutive members share launches
// --, one copy of the info words and one synchronisation per round.  A member whose ladder ends without a factor keeps running through the later launches
// on whatever its buffers hold (no index depends on a value); its numbers are dropped and its outputs are NaN.
// Buffers: g->dSpBatch / dSpBatchAux, carved below, operand group by operand group with the members side by side.  Nothing of
// the context's sparse state (g->sp), of the exact model or of the exact batch is read or written; no validity flag moves.
#include "api_internal.h"

#define GP_SPB_MAX_R 64
// per member in `out` (doubles): the scalars, log det B, the hyper-parameter sums of the Knm and the Kmm pass, dZ of both passes
enum { SPB_SCAL = 0, SPB_LOGDET = 8, SPB_HYP_NM = 16, SPB_HYP_MM = 16 + 4 * GP_SPARSE_NH, SPB_DZ = 160 };
static_assert(GP_MAX_D / GP_GRAD_CH * GP_SPARSE_NH <= 4 * GP_SPARSE_NH && SPB_HYP_MM + 4 * GP_SPARSE_NH <= SPB_DZ, "out: the slots do not overlap");
enum { SPB_TAB_BETA = 0, SPB_TAB_HBETA, SPB_TAB_BETA2, SPB_TAB_JIT, SPB_TAB_DIAG, SPB_TAB_TRACE, SPB_TAB_TRACE2, SPB_NTAB };

// where everything lives in dSpBatch for R members (offsets and strides in doubles)
struct SpbLayout {
    long n, sK, sI, sT, sR, sVec, sPart, sOut, sZ;
    long Kmm, Bm, InvM, InvB, LmiT, Lmi, LbiT, Lbi, VVt, Dm, E, DKmm, Tmp, Tmp2, Kfu, V, Wt, Vec, Part, Out, Tab, Z, total;
    size_t kp_bytes, aux_bytes;
};
static SpbLayout spb_layout(const gp_ctx *g, int R, long Mz) {
    SpbLayout L;
    const long n = round_up(Mz, GP_TILE), Npad = g->Npad;
    L.n = n;
    L.sK = (n + GP_TILE) * n;
    L.sI = n * GP_TILE;
    L.sT = n * n;
    L.sR = Npad * n;
    L.sVec = 4L * g->P * n;
    L.sPart = std::max(sparse_grad_partial_elems(n, g->N), sparse_grad_partial_elems(n, Mz));
    L.sOut = round_up(SPB_DZ + 2 * Mz * g->D, 2);
    L.sZ = Mz * g->D;
    long at = 0;
    auto take = [&](long &off, long stride) { off = at; at += stride * R; };
    take(L.Kmm, L.sK);
    take(L.Bm, L.sK);
    take(L.InvM, L.sI);
    take(L.InvB, L.sI);
    for (long *o : {&L.LmiT, &L.Lmi, &L.LbiT, &L.Lbi, &L.VVt, &L.Dm, &L.E, &L.DKmm, &L.Tmp, &L.Tmp2}) take(*o, L.sT);
    for (long *o : {&L.Kfu, &L.V, &L.Wt}) take(*o, L.sR);
    take(L.Vec, L.sVec);
    take(L.Part, L.sPart);
    take(L.Out, L.sOut);
    take(L.Tab, SPB_NTAB);   // (every block above is a whole number of 16-byte pairs; the odd ones come last)
    take(L.Z, L.sZ);
    L.total = at;
    L.kp_bytes = (sizeof(KernParams) * R + 255) / 256 * 256;
    L.aux_bytes = L.kp_bytes + sizeof(int) * 4 * R;
    return L;
}

// the checks both entries share; nothing is allocated or launched
static int spb_check(gp_ctx *g, int R, int64_t Mz) {
    GP_DEAD_CHECK(g);
    GP_NO_MEAN(g, "gp_sparse_fit_grad_batch");
    if (!g->have_data || !g->have_params) return fail(GP_ERR_STATE, "set data and params before gp_sparse_fit_grad_batch");
    if (g->kp.gower) return fail(GP_ERR_STATE, "the sparse GP does not take the Gower option");
    if (g->warp.n > 0) return fail(GP_ERR_STATE, "the sparse GP does not take an output warp (gp_set_output_warp)");
    if (R < 1 || R > GP_SPB_MAX_R) return fail(GP_ERR_ARG, "gp_sparse_fit_grad_batch takes 1..%d members (got %d)", GP_SPB_MAX_R, R);
    if (Mz < 1 || Mz > GP_SPARSE_MAX_INDUCING) return fail(GP_ERR_ARG, "Mz out of range (1..%d)", GP_SPARSE_MAX_INDUCING);
    return 0;
}

extern "C" int gp_sparse_batch_bytes(gp_t *g, int R, int64_t Mz, int64_t *bytes) {
    if (!g || !bytes) return fail(GP_ERR_ARG, "null argument");
    int rc;
    if ((rc = spb_check(g, R, Mz))) return rc;
    const SpbLayout L = spb_layout(g, R, Mz);
    *bytes = (int64_t)L.total * (int64_t)sizeof(double) + (int64_t)L.aux_bytes;
    return 0;
}

extern "C" int gp_sparse_fit_grad_batch(gp_t *g, int R, int64_t Mz, const double *Z, const double *variance, const double *lengthscale,
                                        const double *noise, int maxtries, double *lml, double *jitter_kmm, double *jitter_b,
                                        double *dvariance, double *dlengthscale, double *dnoise, double *dZ, int *status) {
    if (!g || !Z || !variance || !lengthscale || !noise || !lml || !jitter_kmm || !jitter_b || !dvariance || !dlengthscale || !dnoise ||
        !dZ || !status)
        return fail(GP_ERR_ARG, "null argument");
    int rc;
    if ((rc = spb_check(g, R, Mz))) return rc;
    if (g->P > GP_SPARSE_GRAD_MAX_P) return fail(GP_ERR_ARG, "gp_sparse_fit_grad_batch supports P <= %d", GP_SPARSE_GRAD_MAX_P);
    if (sparse_grad_lds_bytes(g->D, g->P) > (size_t)g->lds_per_wg)
        return fail(GP_ERR_ARG, "gp_sparse_fit_grad_batch: D = %d, P = %d need %zu bytes of LDS per workgroup in the gradient pass, the device has %ld",
                    g->D, g->P, sparse_grad_lds_bytes(g->D, g->P), g->lds_per_wg);
    const int D = g->D, P = g->P, nls = g->ard ? D : 1;
    std::vector<KernParams> kp;   // per-member parameters
    if ((rc = member_params(g, R, variance, lengthscale, noise, &kp))) return rc;
    const SpbLayout L = spb_layout(g, R, Mz);
    const int64_t bytes = (int64_t)L.total * (int64_t)sizeof(double) + (int64_t)L.aux_bytes;
    if (bytes > GP_SPARSE_BATCH_MAX_BYTES)
        return fail(GP_ERR_ARG, "gp_sparse_fit_grad_batch: R = %d members of Mz = %ld over N = %ld need %lld bytes, more than GP_SPARSE_BATCH_MAX_BYTES = %lld",
                    R, (long)Mz, g->N, (long long)bytes, (long long)GP_SPARSE_BATCH_MAX_BYTES);
    HIPCHK(hipSetDevice(g->device));
    if ((rc = g->dSpBatch.reserve(L.total))) return rc;
    if ((rc = g->dSpBatchAux.reserve((long)L.aux_bytes))) return rc;

    const long n = L.n, N = g->N, Npad = g->Npad;
    const int ntz = (int)(n / GP_TILE), nt = (int)(Npad / GP_TILE);
    hipStream_t s = g->s;
    double *B0 = g->dSpBatch;
    double *Kmm = B0 + L.Kmm, *Bm = B0 + L.Bm, *InvM = B0 + L.InvM, *InvB = B0 + L.InvB, *LmiT = B0 + L.LmiT, *Lmi = B0 + L.Lmi,
           *LbiT = B0 + L.LbiT, *Lbi = B0 + L.Lbi, *VVt = B0 + L.VVt, *Dm = B0 + L.Dm, *E = B0 + L.E, *DKmm = B0 + L.DKmm,
           *Tmp = B0 + L.Tmp, *Tmp2 = B0 + L.Tmp2, *Kfu = B0 + L.Kfu, *V = B0 + L.V, *Wt = B0 + L.Wt, *Vec = B0 + L.Vec,
           *Part = B0 + L.Part, *Out = B0 + L.Out, *Tab = B0 + L.Tab, *dZin = B0 + L.Z;
    double *dBeta = Tab + (long)SPB_TAB_BETA * R, *dHbeta = Tab + (long)SPB_TAB_HBETA * R, *dBeta2 = Tab + (long)SPB_TAB_BETA2 * R,
           *dJit = Tab + (long)SPB_TAB_JIT * R, *dDiag = Tab + (long)SPB_TAB_DIAG * R, *dTrace = Tab + (long)SPB_TAB_TRACE * R;
    KernParams *dKp = (KernParams *)g->dSpBatchAux.p;
    int *dInfo = (int *)(g->dSpBatchAux + L.kp_bytes);
    const long sT = L.sT, sR = L.sR, sK = L.sK, sVec = L.sVec;
    double *vec0 = Vec, *vec1 = vec0 + (long)P * n, *vec2 = vec1 + (long)P * n, *vec3 = vec2 + (long)P * n;

    // the coefficient tables (host arithmetic as the single call's)
    std::vector<double> tab((size_t)SPB_NTAB * R, 0.0), beta(R), diag(R, 1e-8);
    for (int r = 0; r < R; ++r) {
        beta[r] = 1.0 / std::max(noise[r], 1e-8);   // var_dtc.py:80
        tab[(size_t)SPB_TAB_BETA * R + r] = beta[r];
        tab[(size_t)SPB_TAB_HBETA * R + r] = -0.5 * P * beta[r];
        tab[(size_t)SPB_TAB_BETA2 * R + r] = 2.0 * beta[r];
        tab[(size_t)SPB_TAB_DIAG * R + r] = 1e-8;
    }
    HIPCHK(hipMemcpyAsync(dKp, kp.data(), sizeof(KernParams) * R, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(Tab, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dZin, Z, sizeof(double) * L.sZ * R, hipMemcpyHostToDevice, s));
    // the diagonal-tile kernel writes the lower block triangle of each inverted tile only: the blocks above it must be zero
    HIPCHK(hipMemsetAsync(InvM, 0, sizeof(double) * L.sI * 2 * R, s));
    std::vector<int> st(R, 0), active(R, 1);
    std::vector<double> jit_m(R, 0.0), jit_b(R, 0.0);
    Members m;
    m.nb = R;
    m.lda = n;
    m.sA = sK;
    m.sI = L.sI;
    m.info = dInfo;
    m.X = dZin;
    m.sX = L.sZ;
    m.kp = kp.data();
    m.kpt = dKp;
    m.diag = diag.data();
    m.diag_tab = dDiag;
    m.jit_tab = dJit;
    auto nt_square = [&](double *C, const double *A, const double *B) {
        gemm(g, s, 0, C, n, A, n, B, n, 1, (int)n, TileSet{0, ntz, 0, ntz, 0}, member_opt(m, GemmOpt(), sT, sT, sT));
    };
    auto both_sides = [&](double *S, const double *LiT, const double *M) {   // S = L^-T M L^-1 (M symmetric)
        nt_square(Tmp2, LiT, M);
        nt_square(S, Tmp2, LiT);
    };
    auto inverse_T = [&](double *LiT, double *Li, const double *A, const double *invT) {   // L^-T by the solve of the identity, L^-1
        identity_blocks(s, LiT, n, R);
        panel_inv_steps(g, s, LiT, n, A, n, invT, ntz, member_opt(m, GemmOpt(), sT, sT, 0), sK, L.sI);
        launch_transpose_blocks(s, Li, LiT, n, R);
    };
    // behind the matrix build of an attempt of either ladder: the jitter, and the zero RHS tile row below each member's matrix
    auto jitter_rhs = [&](const Members &run, bool jittered) {
        if (jittered) launch_add_diag(s, run.A, n, Mz, run.jit[0], run.nb, run.sA, run.jit_tab);
        HIPCHK(hipMemset2DAsync(run.A + n * n, sizeof(double) * sK, 0, sizeof(double) * GP_TILE * n, run.nb, s));
        return 0;
    };

    // Kmm = K(Z) + const_jitter I (var_dtc.py:93-95), Lm, Lm^-T, Lm^-1
    m.A = Kmm;
    m.invL = InvM;
    m.jit = jit_m.data();
    rc = members_ladder(g, m, ntz, maxtries, active, jit_m, dJit, st,
                        [&](const Members &run, int, bool jittered) {
                            launch_kbuild(s, run.A, n, run.X, Mz, n, run.kp[0], 1e-8, 0, run.nb, run.sA, run.kpt, run.diag_tab, run.sX);
                            return jitter_rhs(run, jittered);
                        },
                        [&](const std::vector<int> &failed, std::vector<double> &d0) {
                            for (int r : failed) d0[r] = kp[r].variance + 1e-8;
                            return 0;
                        });
    if (rc) return rc;
    inverse_T(LmiT, Lmi, Kmm, InvM);
    // psi1 = K(X, Z) (var_dtc.py:125); V = Lm^-1 psi1^T (:130 without sqrt(beta)); A = beta V V^T (:131); B = I + A (:134)
    launch_cross_k(s, Kfu, n, g->dX, N, Npad, dZin, Mz, n, kp[0], R, sR, L.sZ, dKp);
    gemm(g, s, 0, V, Npad, Lmi, n, Kfu, n, 1, (int)n, TileSet{0, ntz, 0, nt, 0}, member_opt(m, GemmOpt(), sR, sT, sR));
    gemm(g, s, 0, VVt, n, V, Npad, V, Npad, 1, (int)Npad, TileSet{0, ntz, 0, ntz, 0}, member_opt(m, GemmOpt(), sT, sR, sR));
    // B's ladder: the members that have an Lm
    for (int r = 0; r < R; ++r) active[r] = st[r] == 0;
    m.A = Bm;
    m.invL = InvB;
    m.jit = jit_b.data();
    rc = members_ladder(g, m, ntz, maxtries, active, jit_b, dJit, st,
                        [&](const Members &run, int m0, bool jittered) {
                            launch_sparse_lincomb(s, run.A, VVt + m0 * sT, 0.0, nullptr, 0.0, 1.0, n, run.nb, sK, sT, 0, dBeta + m0, nullptr);
                            return jitter_rhs(run, jittered);
                        },
                        [&](const std::vector<int> &failed, std::vector<double> &d0) {   // mean diagonal of B = 1 + beta trace(VVt) / Mz
                            std::vector<double> tr(2 * (size_t)R);
                            for (int r : failed) launch_trace(s, VVt + r * sT, n, Mz, dTrace + 2L * r);
                            HIPCHK(hipMemcpyAsync(tr.data(), dTrace, sizeof(double) * 2 * R, hipMemcpyDeviceToHost, s));
                            GP_SYNC(s);
                            for (int r : failed) d0[r] = 1.0 + beta[r] * tr[2 * (size_t)r] / (double)Mz;
                            return 0;
                        });
    if (rc) return rc;
    inverse_T(LbiT, Lbi, Bm, InvB);
    // _LBi_Lmi_psi1Vf, Cpsi1Vf (var_dtc.py:138-142), one row of n per output
    launch_sparse_thin(s, V, Npad, n, N, g->dY, 1, P, P, 0.0, vec0, n, R, sR, 0, sVec, dBeta);
    launch_sparse_thin(s, Lbi, n, n, n, vec0, n, 1, P, 1.0, vec1, n, R, sT, sVec, sVec);
    launch_sparse_thin(s, LbiT, n, n, n, vec1, n, 1, P, 1.0, vec2, n, R, sT, sVec, sVec);
    launch_sparse_thin(s, LmiT, n, n, n, vec2, n, 1, P, 1.0, vec3, n, R, sT, sVec, sVec);
    // DBi_plus_BiPBi = LB^-T (P I + delit) LB^-1 (var_dtc.py:148-150)
    launch_sparse_outer(s, Tmp, vec1, n, P, (double)P, n, R, sT, sVec);
    both_sides(Dm, LbiT, Tmp);
    launch_sparse_scalars(s, g->dY, N * P, VVt, Dm, Mz, n, vec1, P, Out + SPB_SCAL, R, sT, sVec, L.sOut);
    launch_logdet(s, Bm, n, Mz, Out + SPB_LOGDET, R, sK, L.sOut);
    // dL_dKmm = Lm^-T (-0.5 DBi_plus_BiPBi - 0.5 P B + P I) Lm^-1 (var_dtc.py:152-156), B = I + beta VVt
    launch_sparse_lincomb(s, Tmp, Dm, -0.5, VVt, 0.0, 0.5 * P, n, R, sT, sT, sT, nullptr, dHbeta);
    both_sides(DKmm, LmiT, Tmp);
    // dL_dpsi2_beta = 0.5 Lm^-T (P I - DBi_plus_BiPBi) Lm^-1 (var_dtc.py:221); Wt = psi1 dL_dpsi2_beta (:232 without 2 beta)
    launch_sparse_lincomb(s, Tmp, Dm, -0.5, nullptr, 0.0, 0.5 * P, n, R, sT, sT, 0);
    both_sides(E, LmiT, Tmp);
    gemm(g, s, 0, Wt, n, Kfu, n, E, n, 1, (int)n, TileSet{0, nt, 0, ntz, 0}, member_opt(m, GemmOpt(), sR, sR, sT));
    // the Kmm part (gradients_X's tmp + tmp.T: twice the symmetric weight), then the Knm part: dL_dKnm = beta Y w^T + 2 beta Wt
    double *dZmm = Out + SPB_DZ, *dZnm = dZmm + Mz * D;
    SparseGradMembers gm;
    gm.nb = R;
    gm.sZ = gm.sXc = L.sZ;
    gm.sW = sT;
    gm.sP = L.sPart;
    gm.sDZ = gm.sH = L.sOut;
    gm.kpt = dKp;
    launch_sparse_grad(s, dZin, Mz, n, dZin, Mz, kp[0], nullptr, 0, nullptr, 0, 0.0, DKmm, n, 1.0, Part, 2.0, dZmm, Out + SPB_HYP_MM, &gm);
    gm.sXc = 0;
    gm.sC = sVec;
    gm.sW = sR;
    gm.ybeta_tab = dBeta;
    gm.wscale_tab = dBeta2;
    launch_sparse_grad(s, dZin, Mz, n, g->dX, N, kp[0], g->dY, P, vec3, n, 0.0, Wt, n, 0.0, Part, 1.0, dZnm, Out + SPB_HYP_NM, &gm);
    std::vector<double> out((size_t)L.sOut * R);
    HIPCHK(hipMemcpyAsync(out.data(), Out, sizeof(double) * out.size(), hipMemcpyDeviceToHost, s));
    GP_SYNC(s);

    const double nan = std::nan("");
    for (int r = 0; r < R; ++r) {
        status[r] = st[r];
        double *dl = dlengthscale + (long)r * nls, *dz = dZ + (long)r * L.sZ;
        if (st[r]) {
            lml[r] = jitter_kmm[r] = jitter_b[r] = dvariance[r] = dnoise[r] = nan;
            std::fill(dl, dl + nls, nan);
            std::fill(dz, dz + L.sZ, nan);
            continue;
        }
        const double *o = out.data() + (size_t)L.sOut * r, *sc = o + SPB_SCAL;
        const double b = beta[r];
        const double trYYT = sc[0], trA = b * sc[1], data_fit = sc[2], sumAD = b * sc[3], logdetB = o[SPB_LOGDET];
        const double psi0_sum = (double)N * kp[r].variance, NP = (double)N * P;
        // _compute_log_marginal_likelihood (var_dtc.py:266-277)
        const double lik_1 = -0.5 * NP * (std::log(2.0 * M_PI) - std::log(b)) - 0.5 * b * trYYT;
        const double lik_2 = -0.5 * P * (b * psi0_sum - trA);
        const double lik_3 = -(double)P * 0.5 * logdetB;
        const double lik_4 = 0.5 * data_fit;
        lml[r] = lik_1 + lik_2 + lik_3 + lik_4;
        // _compute_dL_dR (var_dtc.py:261-263)
        double dR = -0.5 * NP * b + 0.5 * trYYT * b * b;
        dR += 0.5 * P * (psi0_sum * b * b - trA * b);
        dR += b * (0.5 * sumAD - data_fit);
        dnoise[r] = dR;
        jitter_kmm[r] = jit_m[r];
        jitter_b[r] = jit_b[r];
        const double *hnm = o + SPB_HYP_NM, *hmm = o + SPB_HYP_MM;
        // sparse_gp.py:110-115: the diagonal part (dL_dKdiag = -0.5 P beta per row: variance only), the Knm part, the Kmm part
        dvariance[r] = -0.5 * P * b * (double)N + hnm[0] / kp[r].variance + hmm[0] / kp[r].variance;   // stationary.py:224
        double iso = 0.0;
        for (int d = 0; d < D; ++d) {   // -sum W g d_q^2 / l_q (stationary.py:230-238)
            const int at = (d / GP_GRAD_CH) * GP_SPARSE_NH + 1 + d % GP_GRAD_CH;
            const double v = -hnm[at] / kp[r].ls[d] + -hmm[at] / kp[r].ls[d];
            if (g->ard) dl[d] = v;
            iso += v;
        }
        if (!g->ard) dl[0] = iso;
        // sparse_gp.py:117-118
        const double *zmm = o + SPB_DZ, *znm = zmm + Mz * D;
        for (long e = 0; e < Mz * D; ++e) dz[e] = zmm[e] + znm[e];
    }
    return 0;
}
