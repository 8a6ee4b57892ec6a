// Entropy search (GPyOpt/GPyOpt/acquisitions/ES.py, util/epmgp.py): the EP sweeps of p_min, one workgroup per chain, and the
// scoring of candidates against a resident belief.  Always true fp64; every reduction has a fixed order, no atomics.
#include "rows_body.h"
#include "../../include/gphip.h"

#define ES_EP_THREADS 256
#define ES_TILE 16           // candidates per workgroup of the scoring kernel: four waves of four
#define ES_PER_WAVE 4

// numpy.max of two values: a NaN wins (fmax would drop it)
__device__ __forceinline__ double es_npmax(double a, double b) { return (a != a || b != b) ? (a + b) : (a > b ? a : b); }

// ---- EP: min_faktor's sweeps (epmgp.py:122-153) with lt_factor (:211-272) and log_relative_gauss (:276-288) ----------------
// Chain k asks "representer k is the minimum": R - 1 half-space factors (f_l - f_k) / sqrt2 >= 0, visited in index order.  The
// chain's working mean M and covariance V live in LDS.  Every lane derives a step's scalars from the same LDS words, so every
// branch is uniform; the rank-one update of V is spread over the workgroup.  At most max_sweeps (R - 1) steps, no waiting.
// status: 0 converged (sum |d| < tol), 1 sweep limit, -1 a factor gave exit_flag -1 / a NaN d (the reference: logZ = -inf),
// -2 NaN in V (the reference raises).  sweeps: sweeps begun.
__global__ __launch_bounds__(ES_EP_THREADS) void es_pmin_kernel(const double *__restrict__ mu, const double *__restrict__ cov, int R,
                                                                 int max_sweeps, double tol, double *__restrict__ Pout,
                                                                 double *__restrict__ MPout, double *__restrict__ logSout,
                                                                 int *__restrict__ status, int *__restrict__ sweeps) {
    __shared__ double V[GP_ES_MAX_R * GP_ES_MAX_R];
    __shared__ double Mv[GP_ES_MAX_R], Vc[GP_ES_MAX_R], P[GP_ES_MAX_R], MP[GP_ES_MAX_R], LS[GP_ES_MAX_R];
    __shared__ int nanflag;
    const int k = blockIdx.x, t = threadIdx.x;
    const double sq2 = 1.4142135623730951, l2p = 1.8378770664093453, eps = 1.1920928955078125e-07;
    for (int e = t; e < R * R; e += ES_EP_THREADS) V[e] = cov[e];
    if (t < R) {
        Mv[t] = mu[t];
        P[t] = MP[t] = LS[t] = 0.0;
    }
    if (t == 0) nanflag = 0;
    __syncthreads();
    int st = 1, count = 0;
    bool stop = false;
    for (; count < max_sweeps && !stop; ++count) {
        double diff = 0.0;
        for (int i = 0; i < R - 1; ++i) {
            const int l = i < k ? i : i + 1;
            const double p = P[i], mp = MP[i];
            const double cVc = (V[l * R + l] - 2.0 * V[k * R + l] + V[k * R + k]) / 2.0;
            const double cM = (Mv[l] - Mv[k]) / sq2;
            const double cVnic = es_npmax(cVc / (1.0 - p * cVc), 0.0);
            const double cmni = cM + cVnic * (p * cM - mp);
            double z = cmni / sqrt(cVnic + 1e-25);
            if (z != z) z = -INFINITY;
            double pnew, mpnew, logS, d, dp, dmp;
            if (z < -6.0) {   // exit_flag -1
                __syncthreads();
                if (t == 0) {
                    P[i] = 0.0;
                    MP[i] = 0.0;
                    LS[i] = -INFINITY;
                }
                st = -1;
                stop = true;
                break;
            }
            if (z > 6.0) {    // exit_flag 1: the message is removed
                pnew = 0.0;
                mpnew = 0.0;
                dp = -p;
                dmp = -mp;
                d = dp > dmp ? dp : dmp;
                logS = 0.0;
            } else {
                const double logphi = -0.5 * (z * z + l2p);
                const double logPhi = log(0.5 * erfc(-z / sq2));
                const double e = exp(logphi - logPhi);
                const double alpha = e / sqrt(cVnic);
                const double beta = alpha * (alpha * cVnic + cmni);
                const double r = beta / (1.0 - beta);
                pnew = r / cVnic;
                mpnew = r * (alpha + cmni / cVnic) + alpha;
                dp = es_npmax(-p + eps, pnew - p);
                dmp = es_npmax(-mp + eps, mpnew - mp);
                d = es_npmax(dmp, dp);
                pnew = p + dp;
                mpnew = mp + dmp;
                logS = logPhi - 0.5 * (log(beta) - log(pnew) - log(cVnic)) + (alpha * alpha) / (2.0 * beta) * cVnic;
            }
            const double den = 1.0 + dp * cVc;
            const double cV = dp / den, cMu = (dmp - cM * dp) / den;
            __syncthreads();   // every lane has read this step's scalars
            if (t < R) Vc[t] = (V[t * R + l] - V[t * R + k]) / sq2;
            if (t == 0) {
                P[i] = pnew;
                MP[i] = mpnew;
                LS[i] = logS;
            }
            __syncthreads();
            bool bad = false;
            for (int e = t; e < R * R; e += ES_EP_THREADS) {
                const int a = e / R, b = e - a * R;
                const double v = V[e] - cV * (Vc[a] * Vc[b]);
                V[e] = v;
                bad |= (v != v);
            }
            if (t < R) Mv[t] += cMu * Vc[t];
            if (bad) nanflag = 1;   // every writer stores the same word
            __syncthreads();
            if (nanflag) {
                st = -2;
                stop = true;
                break;
            }
            if (d != d) {
                st = -1;
                stop = true;
                break;
            }
            diff += fabs(d);
        }
        if (!stop && fabs(diff) < tol) {
            st = 0;
            stop = true;
        }
    }
    __syncthreads();
    if (t < R - 1) {
        Pout[(long)k * (R - 1) + t] = P[t];
        MPout[(long)k * (R - 1) + t] = MP[t];
        logSout[(long)k * (R - 1) + t] = LS[t];
    }
    if (t == 0) {
        status[k] = st;
        sweeps[k] = count;
    }
}

void launch_es_pmin(hipStream_t s, const double *mu, const double *cov, int R, int max_sweeps, double tol, double *P, double *MP,
                    double *logS, int *status, int *sweeps) {
    GP_LAUNCH(es_pmin_kernel, dim3((unsigned)R), dim3(ES_EP_THREADS), 0, s, mu, cov, R, max_sweeps, tol, P, MP, logS, status, sweeps);
}

// ---- scoring (ES.py:124-170 with _innovations :175-207) -----------------------------------------------------------------------
// C [mc, ldc]: posterior covariance between candidate c and the representers, latent units; var [mc]: the candidate's latent
// variance without noise.  Per candidate: m = C y_std^2 / sqrt(max(var y_std^2, 1e-10)), det_i = m^T Q_i m, g_i = G_i . m, then for
// each quantile w the log-sum-exp over i of logP_i + det_i + g_i w and dHp(w); out = -mean_w dHp.  Qt [R, R, R] and Gt [R, R] are
// stored with the belief index LAST, so that lane i of a wave reads consecutive words; a wave owns ES_PER_WAVE candidates whose m
// it reads from LDS (one address per wave), so each word of Q serves four candidates.  Sums run in index order; the mean over w is
// a strided partial per thread and a fixed tree: a candidate's value depends on nothing but its own row of C and var.
struct EsTile {   // a workgroup's LDS for ES_TILE candidates
    double m[ES_TILE][GP_ES_MAX_R], base[ES_TILE][GP_ES_MAX_R], gl[ES_TILE][GP_ES_MAX_R];
    double Ws[GP_ES_MAX_S], us[GP_ES_MAX_R], red[256];
    int infflag;
};
// The scores of the first nc candidates of the tile, whose innovations L.m holds (zero rows beyond nc, zero entries beyond R), into
// out[0 .. nc).  Called by all 256 threads of the workgroup.
__device__ __forceinline__ void es_score_tile(EsTile &L, int nc, int R, const double *__restrict__ Qt, const double *__restrict__ Gt,
                                              const double *__restrict__ logP, const double *__restrict__ u,
                                              const double *__restrict__ W, int S, double *__restrict__ out) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int e = t; e < S; e += 256) L.Ws[e] = W[e];
    if (t < R) L.us[t] = u[t];
    __syncthreads();
    if (lane < R && wave * ES_PER_WAVE < nc) {
        const int i = lane, cb = wave * ES_PER_WAVE;
        double det[ES_PER_WAVE] = {0.0, 0.0, 0.0, 0.0}, g[ES_PER_WAVE] = {0.0, 0.0, 0.0, 0.0};
        for (int a = 0; a < R; ++a) {
            double row[ES_PER_WAVE] = {0.0, 0.0, 0.0, 0.0};
            for (int b = 0; b < R; ++b) {
                const double q = Qt[((long)a * R + b) * R + i];
#pragma unroll
                for (int j = 0; j < ES_PER_WAVE; ++j) row[j] += q * L.m[cb + j][b];
            }
            const double ga = Gt[(long)a * R + i];
#pragma unroll
            for (int j = 0; j < ES_PER_WAVE; ++j) {
                det[j] += row[j] * L.m[cb + j][a];
                g[j] += ga * L.m[cb + j][a];
            }
        }
        const double lp = logP[i];
#pragma unroll
        for (int j = 0; j < ES_PER_WAVE; ++j) {
            L.base[cb + j][i] = lp + det[j];
            L.gl[cb + j][i] = g[j];
        }
    }
    __syncthreads();
    for (int c = 0; c < nc; ++c) {   // uniform: nc is the workgroup's
        if (t == 0) L.infflag = 0;
        __syncthreads();
        // first pass: does any quantile's normaliser come out infinite?  (ES.py:162-163 then takes the maximum for all of them)
        bool anyinf = false;
        for (int w = t; w < S; w += 256) {
            const double ww = L.Ws[w];
            double mx = -INFINITY;
            for (int i = 0; i < R; ++i) mx = es_npmax(mx, L.base[c][i] + L.gl[c][i] * ww);
            double se = 0.0;
            for (int i = 0; i < R; ++i) se += exp(L.base[c][i] + L.gl[c][i] * ww - mx);
            const double lse = mx + log(se);
            anyinf |= (lse == INFINITY || lse == -INFINITY);
        }
        if (anyinf) L.infflag = 1;   // every writer stores the same word
        __syncthreads();
        const bool usemax = L.infflag != 0;
        double part = 0.0;
        for (int w = t; w < S; w += 256) {
            const double ww = L.Ws[w];
            double mx = -INFINITY;
            for (int i = 0; i < R; ++i) mx = es_npmax(mx, L.base[c][i] + L.gl[c][i] * ww);
            double norm = mx;
            if (!usemax) {
                double se = 0.0;
                for (int i = 0; i < R; ++i) se += exp(L.base[c][i] + L.gl[c][i] * ww - mx);
                norm = mx + log(se);
            }
            double dh = 0.0;
            for (int i = 0; i < R; ++i) {
                const double l = L.base[c][i] + L.gl[c][i] * ww - norm;
                dh += exp(l) * (l + L.us[i]);
            }
            part += dh;
        }
        L.red[t] = part;
        __syncthreads();
        for (int h = 128; h > 0; h >>= 1) {
            if (t < h) L.red[t] += L.red[t + h];
            __syncthreads();
        }
        if (t == 0) out[c] = -(L.red[0] / (double)S);
        __syncthreads();
    }
}

// the innovation of a candidate towards representer r: c the latent covariance between them, var the candidate's latent variance
// without noise, floored at 1e-10 once un-normalised (gpmodel.py:99 through ES.py:199)
__device__ __forceinline__ double es_innovation(double c, double var, double y_std) {
    return c * (y_std * y_std) / sqrt(fmax(var * y_std * y_std, 1e-10));
}

__global__ __launch_bounds__(256) void es_score_kernel(const double *__restrict__ C, long ldc, const double *__restrict__ var, long mc,
                                                        double y_std, int R, const double *__restrict__ Qt,
                                                        const double *__restrict__ Gt, const double *__restrict__ logP,
                                                        const double *__restrict__ u, const double *__restrict__ W, int S,
                                                        double *__restrict__ out) {
    __shared__ EsTile L;
    const int t = threadIdx.x;
    const long c0 = (long)blockIdx.x * ES_TILE;
    for (int e = t; e < ES_TILE * GP_ES_MAX_R; e += 256) {
        const int c = e / GP_ES_MAX_R, r = e - c * GP_ES_MAX_R;
        L.m[c][r] = (c0 + c < mc && r < R) ? es_innovation(C[(c0 + c) * ldc + r], var[c0 + c], y_std) : 0.0;
    }
    es_score_tile(L, (int)min((long)ES_TILE, mc - c0), R, Qt, Gt, logP, u, W, S, out + c0);
}

void launch_es_score(hipStream_t s, const double *C, long ldc, const double *var, long mc, double y_std, int R, const double *Qt,
                     const double *Gt, const double *logP, const double *u, const double *W, int S, double *out) {
    if (mc <= 0) return;
    GP_LAUNCH(es_score_kernel, dim3((unsigned)((mc + ES_TILE - 1) / ES_TILE)), dim3(256), 0, s, C, ldc, var, mc, y_std, R, Qt, Gt, logP,
              u, W, S, out);
}

// ---- a handful of locations: the score behind the fused rows path's forward pass (onerow.hip) -------------------------------------
// The forward pass left w_m = L^-1 k*_m as chunk partials wpart[C][m][n] (rows_body.h).  Workgroup b takes the ES_ROWS_NB entries of
// w from n0 = b ES_ROWS_NB: sums their partials in chunk order, then cpart[b][m][r] = sum_n V_R[r, n] w_m[n] and the |w_m|^2 share,
// each with one writer.  The last workgroup to arrive adds the shares in workgroup order, forms C = k(x_m, xr_r) - V_R w_m and the
// variance kss - |w_m|^2, and scores the locations with the table kernel's arithmetic (es_score_tile) into the pinned block at
// [2 MV + m], the acquisition's place in the rows layout.  Per location the operations and their order are the same whatever
// its slot and the pass's width.
#define ES_ROWS_NB 256
__global__ __launch_bounds__(256) void es_rows_kernel(RowsX rx, KernParams kp, const double *__restrict__ Xr, int R,
                                                       const double *__restrict__ VR, long Npad, const double *__restrict__ wpart, int MV,
                                                       double *__restrict__ cpart, double kss, double y_std,
                                                       const double *__restrict__ Qt, const double *__restrict__ Gt,
                                                       const double *__restrict__ logP, const double *__restrict__ u,
                                                       const double *__restrict__ W, int S, unsigned int *counter,
                                                       unsigned int counter_base, double *out, double ticket) {
    __shared__ EsTile L;
    __shared__ double w_s[ROWS_WIDE_M][ES_ROWS_NB];
    __shared__ double red[4], var_s[ROWS_WIDE_M];
    __shared__ int last_s;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int M = rx.M, D = kp.D;
    const unsigned nblk = gridDim.x, b = blockIdx.x;
    const long n = (long)b * ES_ROWS_NB + t;
    double *mine = cpart + (long)b * ROWS_WIDE_M * (GP_ES_MAX_R + 1);   // [m][r], then the |w_m|^2 shares
    {
        const bool live = n < Npad;
        const int nch = rw_nch((int)((live ? n : 0) / GP_TILE));
        for (int m = 0; m < M; ++m) {
            double s = 0.0;
            if (live)
                for (int C = 0; C < nch; ++C) s += wpart[((long)C * MV + m) * Npad + n];
            w_s[m][t] = s;
            const double q = rw_block_sum(s * s, red);
            if (t == 0) mine[ROWS_WIDE_M * GP_ES_MAX_R + m] = q;
        }
    }
    __syncthreads();
    for (int r = wave; r < R; r += 4) {
        const double *row = VR + (long)r * Npad + (long)b * ES_ROWS_NB;
        double v[ES_ROWS_NB / 64];
#pragma unroll
        for (int q = 0; q < ES_ROWS_NB / 64; ++q) v[q] = ((long)b * ES_ROWS_NB + lane + 64 * q < Npad) ? row[lane + 64 * q] : 0.0;
        for (int m = 0; m < M; ++m) {
            double a = 0.0;
#pragma unroll
            for (int q = 0; q < ES_ROWS_NB / 64; ++q) a = fma(v[q], w_s[m][lane + 64 * q], a);
            a = rw_wave_sum(a);
            if (lane == 0) mine[m * GP_ES_MAX_R + r] = a;
        }
    }
    __threadfence();
    __syncthreads();
    if (t == 0) last_s = (atomicAdd(counter, 1u) - counter_base == nblk - 1) ? 1 : 0;   // (unsigned: wraps with the base)
    __syncthreads();
    if (!last_s) return;
    __threadfence();
    if (t < M) {
        double s = 0.0;
        for (unsigned k = 0; k < nblk; ++k) s += cpart[(long)k * ROWS_WIDE_M * (GP_ES_MAX_R + 1) + ROWS_WIDE_M * GP_ES_MAX_R + t];
        var_s[t] = kss - s;
    }
    __syncthreads();
    for (int e = t; e < ES_TILE * GP_ES_MAX_R; e += 256) {
        const int m = e / GP_ES_MAX_R, r = e - m * GP_ES_MAX_R;
        double val = 0.0;
        if (m < M && r < R) {
            // k(x_m, xr_r): the arithmetic of the forward pass's k* (inputs divided first, squares summed in dimension order)
            double acc = kp.gower ? 1.0 : 0.0;
            for (int d = 0; d < D; ++d) {
                const double df = rx.xs[m * D + d] / kp_div(kp, d) - Xr[r * D + d] / kp_div(kp, d);
                if (kp.gower) {
                    const double rr = kp.gdisc[d] ? (df != 0.0 ? 1.0 : 0.0) : fabs(df);
                    acc *= gp_k_of_r2(kp.kernel, kp.variance, rr * rr);
                } else {
                    acc = fma(df, df, acc);
                }
            }
            const double kxr = kp.gower ? acc : gp_k_of_r2(kp.kernel, kp.variance, acc);
            double s = 0.0;
            for (unsigned k = 0; k < nblk; ++k) s += cpart[(long)k * ROWS_WIDE_M * (GP_ES_MAX_R + 1) + m * GP_ES_MAX_R + r];
            val = es_innovation(kxr - s, var_s[m], y_std);
        }
        L.m[m][r] = val;
    }
    es_score_tile(L, M, R, Qt, Gt, logP, u, W, S, out + 2 * MV);
    __threadfence_system();
    if (t == 0) out[ROWS_OUT_DOUBLES] = ticket;   // this pass is complete (the host checks the ticket behind the results)
}

unsigned es_rows_grid(long Npad) { return (unsigned)((Npad + ES_ROWS_NB - 1) / ES_ROWS_NB); }
size_t es_rows_part_elems(long Npad) { return (size_t)es_rows_grid(Npad) * ROWS_WIDE_M * (GP_ES_MAX_R + 1); }

void launch_es_rows(hipStream_t s, const RowsX &rx, const KernParams &kp, const double *Xr, int R, const double *VR, long Npad,
                    const double *wpart, double *cpart, double kss, double y_std, const double *Qt, const double *Gt,
                    const double *logP, const double *u, const double *W, int S, const PassReport &r) {
    GP_LAUNCH(es_rows_kernel, dim3(es_rows_grid(Npad)), dim3(256), 0, s, rx, kp, Xr, R, VR, Npad, wpart, rows_layout(rx.M), cpart, kss,
              y_std, Qt, Gt, logP, u, W, S, r.counter, r.base, r.out, r.ticket);
}
