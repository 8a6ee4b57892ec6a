// Shared declarations of the api_*.hip translation units: the context behind gp_t, error helpers, and the internal
// entry points each unit offers the others.  (include/gphip.h is the public C ABI; gphip_internal.h the kernels.)
#pragma once
#include "gphip_internal.h"
#include "warp_math.h"
#include "../../include/gphip.h"

#include <hip/hip_ext.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <type_traits>
#include <vector>

extern thread_local std::string g_err;
int fail(int code, const char *fmt, ...);

#define HIPCHK(x)                                                                                   \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess) return fail(GP_ERR_HIP, "%s -> %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define NCCLCHK(x)                                                                                   \
    do {                                                                                             \
        ncclResult_t r_ = (x);                                                                       \
        if (r_ != ncclSuccess) return fail(GP_ERR_RCCL, "%s -> %s (%s:%d)", #x, ncclGetErrorString(r_), __FILE__, __LINE__); \
    } while (0)
// Drain a stream, then report (and clear) what gp_note_hip recorded since the last report: the point where an entry point's
// results are about to be read.
int gp_pending_error();
#define GP_SYNC(stream)                                                                            \
    do {                                                                                            \
        hipError_t e_ = hipStreamSynchronize(stream);                                               \
        int p_ = gp_pending_error();                                                                \
        if (p_) return p_;                                                                          \
        if (e_ != hipSuccess) return fail(GP_ERR_HIP, "hipStreamSynchronize(%s) -> %s (%s:%d)", #stream, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define GP_ERR_RANGE (-1000)   // internal: an operand of the residue path left the fixed-point range (the caller repeats in fp64)
void gp_clear_stale_note();
#define GP_DEAD_CHECK(g)                                                                            \
    do {                                                                                            \
        gp_clear_stale_note();                                                                      \
        if ((g)->dead)                                                                              \
            return fail(GP_ERR_STATE, "the library was shut down (gp_shutdown): destroy this context and create a new one"); \
    } while (0)

// The preamble of an entry point that works on a fit (GP_FITTED) or scores the resident candidates (GP_SCORING): the context is
// alive, holds what the call needs, and its device is current.  (Null arguments are the entry point's own first check.)
#define GP_READY(g, candidates)                                                                     \
    do {                                                                                            \
        GP_DEAD_CHECK(g);                                                                           \
        if (!(g)->fitted) return fail(GP_ERR_STATE, "gp_fit first");                                \
        if ((candidates) && (g)->M < 1) return fail(GP_ERR_STATE, "gp_set_candidates first");       \
        HIPCHK(hipSetDevice((g)->device));                                                          \
    } while (0)
#define GP_FITTED(g) GP_READY(g, false)
#define GP_SCORING(g) GP_READY(g, true)

// The entries whose prediction side would not add m(x), or that read dY as targets: refused while a mean function is resident,
// before anything is launched or changed
#define GP_NO_MEAN(g, who)                                                                          \
    do {                                                                                            \
        if ((g)->mean.on())                                                                         \
            return fail(GP_ERR_STATE, "%s: not available while a mean function is resident (gp_mean_set(NULL, NULL) clears it)", who); \
    } while (0)

// ---- scratch map ----------------------------------------------------------------------------------------------------------
// Where everything lives in the small device buffers that several units carve up: offset and length (in elements) of every
// slot, in this one place.  gp_create (api_core.hip) reserves the *_CAP of dScal, dRedV and dRedI once; dComm and dLp are
// reserved at their *_CAP by their first user.  Each static_assert below lists slots that can be live in the same call: they
// lie inside the capacity and do not overlap.
struct Slot { long off, len; };
template <size_t n>
constexpr bool slots_ok(const Slot (&s)[n], long cap) {
    for (size_t i = 0; i < n; ++i) {
        if (s[i].off < 0 || s[i].len < 1 || s[i].off + s[i].len > cap) return false;
        for (size_t j = 0; j < i; ++j)
            if (s[i].off < s[j].off + s[j].len && s[j].off < s[i].off + s[i].len) return false;
    }
    return true;
}
#define GP_GRAD_MAX_P 16    // gp_lml_grad / gp_fit_grad: outputs whose alpha . y fit in front of the gradient sums
// ... and D and P are limited JOINTLY by the LDS of a workgroup (gp_ctx::lds_per_wg, 163840 B on gfx950): the fused pass stages
// both tiles of the inputs and of alpha, lml_grad_lds_bytes = 576 + 2048 ((gower ? 2 : 1) D + P) bytes -- D + P <= 79, a Gower
// model 2 D + P <= 79.  lml_grad_lds_check refuses the rest up front (GP_ERR_ARG); gradx and the sparse pass fit at every
// accepted (D, P) on that device and are checked all the same.
#define GP_LP_MAX_NB 256    // rows of a local-penalisation batch
#define GP_EXCLUDE_MAX 256  // excluded rows of gp_acq_lp_argbest
#define GP_COMM_MAX_RANKS 128
// dScal, per member (Members::scal; gp_fit_grad_batch strides its members by SCAL_GRAD's end)
constexpr long SCAL_CAP = 512;
constexpr Slot SCAL_LOGDET{0, 1};
constexpr Slot SCAL_DOT{8, GP_MAX_RHS};                  // alpha . y of each output (alpha_lml)
constexpr Slot SCAL_DOT_GRAD{8, GP_GRAD_MAX_P};          // ... as far as it goes in a call that also takes the gradient
constexpr Slot SCAL_GRAD{64, GP_MAX_D / GP_GRAD_CH * GP_GRAD_NACC};   // GP_GRAD_NACC sums per pass of GP_GRAD_CH dimensions
constexpr Slot SCAL_FIT_RECORD{400, 4};                  // gp_comm_bcast_fit
constexpr Slot SCAL_TRACE{420, 2};                       // trace and smallest diagonal entry, gp_posterior_samples
constexpr Slot SCAL_WARP_LOGJAC{430, 1};                 // sum log f'(y) of the output warp (warp_y_kernel)
constexpr Slot SCAL_WARP_GRAD{431, GP_WARP_NPSI};        // the warp's 3 T + 1 gradient sums (warp_grad_kernel)
static_assert(GP_MAX_D % GP_GRAD_CH == 0, "whole gradient passes");
static_assert(slots_ok({SCAL_LOGDET, SCAL_DOT, SCAL_FIT_RECORD, SCAL_TRACE}, SCAL_CAP), "dScal: a fit of up to GP_MAX_RHS outputs");
static_assert(slots_ok({SCAL_LOGDET, SCAL_DOT_GRAD, SCAL_GRAD, SCAL_FIT_RECORD, SCAL_TRACE}, SCAL_CAP), "dScal: fit and gradient");
static_assert(slots_ok({SCAL_LOGDET, SCAL_DOT_GRAD, SCAL_GRAD, SCAL_FIT_RECORD, SCAL_TRACE, SCAL_WARP_LOGJAC, SCAL_WARP_GRAD}, SCAL_CAP),
              "dScal: fit and gradient of a warped model (gp_fit_grad_warp)");
// dRedV (doubles) and dRedI (rows): the two-level arg-best reduction; what rides beside it
constexpr long REDV_CAP = 512, REDI_CAP = 1024;
constexpr Slot RED_PARTIAL{0, 256};                      // first-level winners, in both buffers (launch_argbest: <= 256 blocks)
constexpr Slot RED_RESULT{256, 1};                       // the winner, in both buffers
constexpr Slot REDV_GATHER_SEND{300, 2};                 // gp_comm_allgather_best: this rank's {value, row} ...
constexpr Slot REDV_GATHER_RECV{304, 200};               // ... and every rank's: 2 * nranks doubles
constexpr Slot REDI_EXCLUDE{300, GP_EXCLUDE_MAX};        // rows masked before the reduction
static_assert(slots_ok({RED_PARTIAL, RED_RESULT, REDV_GATHER_SEND, REDV_GATHER_RECV}, REDV_CAP), "dRedV");
static_assert(slots_ok({RED_PARTIAL, RED_RESULT, REDI_EXCLUDE}, REDI_CAP), "dRedI");
// dComm (doubles; rows travel as 8 bytes in a double's place): the local top-k, or a gather of up to GP_TOPK_MAX records a rank
constexpr long COMM_CAP = 2L * GP_TOPK_MAX * (1 + GP_COMM_MAX_RANKS);
constexpr Slot COMM_TOPK_VAL{0, GP_TOPK_MAX}, COMM_TOPK_ROW{GP_TOPK_MAX, GP_TOPK_MAX};
constexpr Slot COMM_SEND{0, 2 * GP_TOPK_MAX}, COMM_RECV{2 * GP_TOPK_MAX, 2L * GP_TOPK_MAX * GP_COMM_MAX_RANKS};
static_assert(slots_ok({COMM_TOPK_VAL, COMM_TOPK_ROW}, COMM_CAP), "dComm: gp_acq_topk");
static_assert(slots_ok({COMM_SEND, COMM_RECV}, COMM_CAP), "dComm: gathers");
// dLp: the penaliser's batch
constexpr long LP_CAP = (long)GP_LP_MAX_NB * (GP_MAX_D + 2);
constexpr Slot LP_X{0, (long)GP_LP_MAX_NB * GP_MAX_D}, LP_R{LP_X.off + LP_X.len, GP_LP_MAX_NB}, LP_S{LP_R.off + LP_R.len, GP_LP_MAX_NB};
static_assert(slots_ok({LP_X, LP_R, LP_S}, LP_CAP), "dLp");

struct Phase {
    const char *name;
    hipEvent_t e0, e1;
    double flops, bytes;
    bool used;
};
#define MAX_PHASES 16

// One device allocation and its owner.  reserve(n) only ever grows: a no-op while n elements fit, otherwise the old block is
// freed and exactly n elements are allocated -- the contents are NOT kept.  Converts to T * where a launch takes the pointer.
// A buffer that was never reserved makes no HIP call, so a gp_ctx without a device behind it can be built and dropped.
template <class T>
struct DevBuf {
    T *p = nullptr;
    long cap = 0;   // elements
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    operator T *() const { return p; }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    hipError_t alloc(long n) {   // release, then exactly n elements; null and 0 when that fails
        release();
        const hipError_t e = hipMalloc((void **)&p, (size_t)n * sizeof(T));
        if (e == hipSuccess) cap = n; else p = nullptr;
        return e;
    }
    int reserve(long n) { return (n <= cap && p) ? 0 : grow(n); }   // the fast path of the ~40 us *_rows calls stays inline
    __attribute__((noinline)) int grow(long n) {
        const hipError_t e = alloc(n);
        if (e == hipSuccess) return 0;
        return std::is_same<T, double>::value ? fail(GP_ERR_HIP, "hipMalloc(%ld doubles) -> %s", n, hipGetErrorString(e))
                                              : fail(GP_ERR_HIP, "hipMalloc(%ld bytes) -> %s", n * (long)sizeof(T), hipGetErrorString(e));
    }
};

// How a fused rows pass completes, and its one owner.  The last workgroup to arrive at a device counter writes the results into
// a pinned block and the pass's ticket behind them; the counter is never reset, each pass counts from a base the host advances
// by the pass's arrivals.  After the sync the host compares the ticket: a pass that did not complete fails loudly -- counter and
// bases cleared, so that the next call starts clean -- instead of handing back the previous call's numbers.  The exact model, the
// sparse model and the ensemble hold one owner each (gp_ctx::pass, SparseState::pass, EnsState::pass): counters, tickets and
// blocks of their own.  An owner that was never used makes no HIP call (as DevBuf).
#define GP_ENS_MAX_S 64
struct PassOwner {
    const int words;                 // counter words: 1; the ensemble 1 + GP_ENS_MAX_S ([0] members arrived, [1 + z] member z's workgroups)
    const char *const who;           // the error text's subject
    DevBuf<unsigned int> counter;
    unsigned int base[2] = {0, 0};   // arrivals the words hold from the passes so far: of the (members') workgroups, of the ensemble's members
    double *block = nullptr;         // pinned, device-visible: ROWS_OUT_DOUBLES results, then the ticket
    double ticket = 0.0;             // counts the passes; the finishing workgroup writes it back
    PassOwner(int words_, const char *who_) : words(words_), who(who_) {}
    ~PassOwner() { if (block) (void)hipHostFree(block); }
    // (api_core.hip) first use: the counter, zeroed on the stream, and the block with its ticket slot at 0
    int ready(hipStream_t s) { return counter && block ? 0 : make_ready(s); }
    int make_ready(hipStream_t s);
    int restart(hipStream_t s);      // every counter word zeroed on the stream, the bases 0 (no-op before the first use)
    PassReport next() { return PassReport{counter, base[0], base[1], block, ticket += 1.0}; }
    // pass r is on the stream with a0 (and a1) arrivals to come: advance the bases, wait, and make sure it finished (see above)
    int wait(hipStream_t s, const PassReport &r, unsigned a0, unsigned a1);
};

// Pinned, device-visible host memory and its owner (as DevBuf: reserve only grows, the contents are not kept)
struct PinBuf {
    double *p = nullptr;
    long cap = 0;
    PinBuf() = default;
    PinBuf(const PinBuf &) = delete;
    PinBuf &operator=(const PinBuf &) = delete;
    ~PinBuf() { if (p) (void)hipHostFree(p); }
    int reserve(long n) {
        if (n <= cap && p) return 0;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        const hipError_t e = hipHostMalloc((void **)&p, (size_t)n * sizeof(double), hipHostMallocDefault);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(GP_ERR_HIP, "hipHostMalloc(%ld doubles) -> %s", n, hipGetErrorString(e));
        }
        cap = n;
        return 0;
    }
};

// The sparse model (variational DTC over Mz inducing inputs, api_sparse.hip) on the context's X, Y, D, P, kernel parameters and
// main stream: buffers and validity flag of its own -- nothing here is read or written by the exact model's entry points, and
// the sparse entry points touch none of the exact model's buffers or flags.  n = Mzpad below.
struct SparseState {
    long Mz = 0, Mzpad = 0;    // inducing inputs set (gp_sparse_set_inducing): Mz > 0
    bool fitted = false;       // the buffers below hold the fit of the current data, parameters and inducing inputs
    bool grad_ready = false;   // ... and dWt / dDKmm hold the gradient weights of that fit
    double lml = 0.0, jitter_kmm = 0.0, jitter_b = 0.0, beta = 0.0, dnoise = 0.0;
    DevBuf<double> dZ;         // [Mz, D]
    DevBuf<double> dZs;        // [Mz, D]: Z / lengthscale of the current fit, built by the first fused rows call after it (sparse_rows.hip)
    bool zs_valid = false;     // dZs belongs to the current fit
    bool fmin_valid = false;   // fmin is the minimum of the training mean under the current fit (gp_sparse_fmin computes it once per fit)
    double fmin = 0.0;
    DevBuf<double> dKmm;       // (n + 128) x n: Kmm -> Lm (lower) with one zero RHS tile row below
    DevBuf<double> dBm;        // (n + 128) x n: B -> LB
    DevBuf<double> dInvT;      // 2 x n x 128: inverted diagonal tiles of Lm, then of LB
    DevBuf<double> dLmiT, dLmi, dLbiT, dLbi;   // n x n: Lm^-T, Lm^-1, LB^-T, LB^-1
    DevBuf<double> dVVt, dDm, dE, dWinv, dDKmm, dTmp, dTmp2;   // n x n: V V^T, DBi_plus_BiPBi, dL_dpsi2_beta, woodbury_inv, dL_dKmm, scratch
    DevBuf<double> dKfu, dV, dWt;        // Npad x n, n x Npad, Npad x n: K(X, Z), Lm^-1 Kuf, Kfu E
    DevBuf<double> dVec;       // 4 x capP x n: V Y, LBi Lmi psi1 Vf, LB^-T of it, the woodbury vector (rows of n per output)
    DevBuf<double> dPartial;   // the gradient pass's slabs
    DevBuf<double> dOut;       // scalars, hyper-parameter sums, dZ of both parts, training mean
    DevBuf<int> dInfo;         // 4 status words of the factorisation in progress
    DevBuf<double> dXs, dKx, dBt, dPred;   // prediction: candidates, K(Xs, Z) and Kx woodbury_inv per chunk, results
    // the resident candidate table of the acquisition entries (gp_sparse_set_candidates) and its lazily cached posterior:
    // buffers of their own, so that gp_sparse_predict and the rows entries between two scoring calls leave them alone
    long tM = 0;               // rows of the table (0: none)
    DevBuf<double> dTab;       // [tM, D]
    DevBuf<double> dTabPost;   // mean [tM], var [tM] (noise included), dmdx [tM, D], dvdx [tM, D]
    DevBuf<double> dTabAcq, dTabDacq;   // scores [tM] and their gradients [tM, D]
    bool tab_post = false, tab_grad = false;   // dTabPost holds mean / var (and the gradients) of the table under the current fit
    // the rows entries: scratch of the fallback (table arithmetic on a handful of rows: locations, posterior, scores) and the
    // fused path's per-workgroup sums and the owner of its passes' completion
    DevBuf<double> dScrX, dScrPost, dScrAcq;
    DevBuf<double> dRowsPart;
    PassOwner pass{1, "the sparse one-location kernel"};
    long rows_fused_calls = 0, rows_fallback_calls = 0;
    // the joint posterior (api_sparse_cov.hip): buffers of its own, nothing of the table cache or of the exact model.  M = rows of
    // the call, Mpad = M rounded up to the tile, R = cR
    DevBuf<double> dCovX;      // [M, D]: the locations of the call
    DevBuf<double> dCovA;      // Mpad x n: K(Xs, Z), then T = U LB^-T; Rpad x n: K(X2, Z) while G is built
    DevBuf<double> dCovU;      // Mpad x n: U = K(Xs, Z) Lm^-T
    DevBuf<double> dCovC, dCovW;   // Mpad x Mpad: the covariance / its factor, T T^T
    DevBuf<double> dCovZ;      // 2 x Spad x Mpad: the caller's normals, the deviations
    DevBuf<double> dCovInv;    // Mpad x 128: inverted diagonal tiles of the covariance's factor
    DevBuf<double> dCovMean;   // P x Mpad: the mean, one row per output
    DevBuf<double> dCovStat;   // trace and smallest diagonal entry of the matrix to factor
    long cR = 0;               // rows of the second point set (gp_sparse_cov_set_points; 0: none)
    DevBuf<double> dX2, dX2s;  // [cR, D]: the points, and the points / lengthscale of the current fit
    DevBuf<double> dG;         // Rpad x n: G = K(X2, Z) woodbury_inv of the current fit, zero rows in the padding
    bool g_valid = false;      // dG and dX2s belong to the current fit and points
    DevBuf<double> dCovOut;    // [M1, cR]: gp_sparse_cov_between beyond ROWS_WIDE_M locations
    PinBuf covPin;             // [ROWS_WIDE_M, cR]: ... and up to that many, written by the kernel
    PassOwner cov_pass{1, "the sparse covariance kernel"};   // its counter and ticket (the block holds the ticket only)
};

// The ensemble (api_ens.hip): S hyper-parameter members over the context's X, Y -- each with alpha, explicit inverse factor,
// parameters, jitter and fmin of its own -- kept beside the context's own fit and independent of it: nothing here is read or
// written by the other entry points (gp_set_data alone drops it), and the ensemble entries leave the context's fit, candidates'
// posterior and parameters as they were.
struct EnsState {
    int S = 0;                 // members of the valid ensemble (0: none)
    DevBuf<double> dLi;        // [S] Npad x Npad inverse factors (lower, row-major, zeros above the diagonal)
    DevBuf<double> dAlpha;     // [S] Npad
    DevBuf<double> dTab;       // noise [S], fmin [S]
    DevBuf<signed char> dKp;   // KernParams [S]
    DevBuf<double> dWork;      // the rows passes' partials per member, then the members' result blocks
    PassOwner pass{1 + GP_ENS_MAX_S, "the ensemble kernels"};   // the block takes the integrated acquisition
    std::vector<double> noise, fmin, jitter;
    std::vector<KernParams> kp;
    DevBuf<double> dKx, dW, dAcq;    // table route: K_z(Xs, X) and Kx Li_z^T per chunk, the scores
};

// Entropy search (api_es.hip): the representers of a fit and the belief over them.  R > 0 while dVR / dXr belong to the factor
// in dA; everything that drops or changes the factor drops both (factor_results_dropped, factor_grown).
struct EsState {
    int R = 0;                 // representers resident (0: none)
    int S = 0;                 // quantiles of the belief
    bool belief = false;       // dBelief holds a belief over the R representers
    DevBuf<double> dXr;        // [R, D]
    DevBuf<double> dVR;        // 128 x Npad: row r = L^-1 K(X, xr_r), zero rows and columns in the padding
    DevBuf<double> dBelief;    // logP [64], u [64], Gt [64 x 64], W [1024], Qt [R^3] (belief index last)
    DevBuf<double> dC;         // mc_pad x 128: a chunk's covariance candidate x representer
    DevBuf<double> dEp;        // gp_es_pmin: mu, cov, P, MP, logS, then status / sweeps words
    DevBuf<double> dRowsPart;  // gp_es_acq_rows: the workgroups' shares of V_R w and |w|^2 (es_rows_part_elems)
};

// The cost surface (api_cost.hip): a snapshot of a cost GP's posterior mean -- inputs over lengthscale, alpha, kernel parameters,
// normaliser -- in buffers of the context's own; nothing of the handle it came from is kept.  Nc > 0 while one is resident.  The
// fit, the posterior caches and the candidates do not depend on it; the cached logc of a resident table does (gp_ctx::cost_tab).
struct CostState {
    long Nc = 0;
    int ld = 0;                // doubles between two rows of dXcs: max(D, 8), zeros beyond D
    KernParams kp{};           // kernel, D, variance, lengthscales of the cost GP (never Gower)
    double shift = 0.0, scale = 1.0;   // m_c = shift + scale K alpha: the cost model's output normaliser
    DevBuf<double> dXcs, dAlpha;       // [Nc, ld], [Nc]
    DevBuf<double> dTabLogc;   // logc of the resident table gp_ctx::cost_tab names
    DevBuf<double> dWork;      // rows not in a resident table: locations [M, D], logc [M], dlogc [M, D]; dlogc of a table
    DevBuf<double> dPart;      // the chunks' partial sums of a values-only table launch cut along the surface (cost.hip)
};

// The probability of feasibility over the resident candidates (api_feas.hip): log prod_k Phi of K constraint GPs, a snapshot in a
// buffer of the context's own -- nothing of the constraint handles is kept.  K > 0 while dTabLogF holds the M rows' values.
struct FeasState {
    int K = 0;
    long M = 0;
    DevBuf<double> dTabLogF;   // [M]
    DevBuf<double> dWork;      // gp_fmin_rows: the listed rows (8 bytes each), then their values
};
static_assert(GP_FEAS_MAX == FEAS_MAX_K, "the kernels' argument takes GP_FEAS_MAX constraints");

// Expected hypervolume improvement (api_ehvi.hip): the cell decomposition of the region the observed Pareto front does not
// dominate, on the SCORED handle (objective 0) -- K level arrays behind each other and the cells' packed index pairs, as EhviCells
// (gphip_internal.h) hands them to the kernels.  K > 0 while one is resident.  Raw objective units: no fit, data or candidate call
// touches it.
struct EhviState {
    int K = 0, C = 0;
    int L[EHVI_MAX_K] = {0, 0, 0}, off[EHVI_MAX_K] = {0, 0, 0};
    DevBuf<double> dLevels;          // [sum_k L[k]]
    DevBuf<unsigned int> dCells;     // [C, K]: lo | hi << 16
};
static_assert(GP_EHVI_MAX_OBJ == EHVI_MAX_K && GP_EHVI_MAX_LEVELS == EHVI_MAX_L, "the kernels' LDS table takes the public caps");

// The affine mean function m(x) = x^T A + b of the exact GP (api_mean.hip): a snapshot of the mapping's parameters in a buffer of
// the context's own.  While one is resident dYraw keeps the targets gp_set_data brought (the output warp's buffer and convention)
// and dY holds the residuals Y - m(X) every fit route factors against; `stale` while dY still has to be rebuilt from them
// (mean_residuals, before the next factorisation).  D and P are the data's.
struct MeanState {
    bool has_A = false, has_b = false;
    bool stale = false;
    DevBuf<double> dAb;        // A [D, P] row-major, then b [P]; an absent part as zeros
    DevBuf<double> dPart;      // gp_mean_grad: the chunks' partial sums, then the (D + 1) P results
    bool on() const { return has_A || has_b; }
};

// Max-value entropy search (api_mes.hip): the caller's K samples of the minimum's value, in a buffer of the context's own, and the
// scratch of the sampler's two reductions.  The samples are the caller's numbers in the caller's units: no fit, data or candidate
// call touches them.
struct MesState {
    int K = 0;                 // samples resident (0: none)
    DevBuf<double> dY;         // [GP_MES_MAX_K]
    DevBuf<double> dPart;      // the chunks' partial sums / minima, then the results (mes_part_elems)
};

// Posterior paths (api_paths.hip): S function samples by pathwise conditioning on the resident factor -- the scaled draws of the
// prior term and the update's weights V.  S > 0 while they belong to the factor in dA; everything that drops or grows the factor
// drops them (factor_results_dropped, factor_grown).
struct PathsState {
    int S = 0, F = 0;          // paths and features resident (0: none)
    int Spad = 0, Fpad = 0;    // ... rounded up to the matrix cores' 16: zero rows / zero weights in the padding
    double amp = 0.0;          // a = sqrt(2 variance / F)
    DevBuf<double> dOmega;     // [Fpad, D]: omega_unit / lengthscale
    DevBuf<double> dPhase;     // [Fpad]
    DevBuf<double> dWt;        // [Spad, Fpad], path-major
    DevBuf<double> dV;         // [Spad, Npad], path-major: one path's column of V is contiguous
    DevBuf<double> dR, dZ;     // 128 x Npad each: z_eps -> the residuals (the solve's running right-hand side), the forward solve
    DevBuf<double> dTab;       // [S, M]: the table of gp_paths_table / gp_paths_argbest
    DevBuf<double> dPart;      // ... and its partial sums over chunks of the training rows (paths_table_part_elems)
    DevBuf<double> dRedV;      // the arg-best reduction's first-level winners and results, per path
    DevBuf<long long> dRedI;
    DevBuf<double> dRows;      // gp_paths_rows: the chunks' partial sums
    PassOwner pass{1, "the path kernel"};   // completion of gp_paths_rows
};

// Joint expected improvement (api_qei.hip): the caller's base samples, in a buffer of the context's own, and what the joint step
// leaves the closing pass.  The samples are standard normals that belong to no fit: no fit, parameter, data or append call touches
// them (common random numbers across refits); they go with the handle.
struct QeiState {
    int S = 0, q = 0;          // samples and columns resident (0: none)
    DevBuf<double> dZ;         // [q, S]: column-major, a column of the caller's Z contiguous
    DevBuf<double> dState;     // QEI_STATE_DOUBLES: status, mbar, A (qei.hip)
    long calls = 0, grad_calls = 0;   // gp_qei_rows calls answered since the context was created, and those with a gradient (gp_qei_stats)
};

// The knowledge gradient (api_kg.hip): the discretisation points of a fit.  A > 0 while dVA / dMuA / dXa belong to the factor in dA;
// everything that drops ES's representers drops them (factor_results_dropped, factor_grown).  Nothing is shared with EsState.
struct KgState {
    int A = 0;                 // discretisation points resident (0: none)
    DevBuf<double> dXa;        // [A, D]
    DevBuf<double> dVA;        // 256 x Npad: row i = L^-1 K(X, a_i), zero rows and columns in the padding
    DevBuf<double> dMuA;       // [A]: the points' latent posterior means
    DevBuf<double> dC;         // mc_pad x 256: a chunk's covariance candidate x point
    DevBuf<double> dRowsPart;  // gp_kg_rows: the workgroups' shares of V_A w and |w|^2 (kg_rows_part_elems)
    DevBuf<double> dState;     // gp_kg_rows: ROWS_WIDE_M state rows of KG_STATE_STRIDE doubles (kg.hip)
};

// Noisy expected improvement (api_nei.hip), resident on the TWIN: S fantasies of the noiseless training values drawn through the
// model's factor and this context's.  S > 0 while the blocks belong to the factor in dA (factor_results_dropped and factor_grown
// drop them) and to the model's fit: `model` is looked up among the live contexts and its fit_gen compared before every use.
struct gp_ctx;
struct NeiState {
    int S = 0;
    double d = 0.0, d0 = 0.0;  // the diagonals of the two factors: noise + 1e-8 + jitter of the model, of the twin
    gp_ctx *model = nullptr;   // never dereferenced before nei_model_unchanged found it alive
    unsigned long long model_gen = 0;
    DevBuf<double> dA0;        // [NEI_SPAD, Npad] fantasy-major: a_s = K0^-1 F_s, zero rows and columns in the padding
    DevBuf<double> dU;         // [128, Npad]: U_s = L0^-1 F_s, the forward substitution's result (the gradient's mix reads it)
    DevBuf<double> dF;         // [NEI_SPAD, Npad]: the fantasies
    DevBuf<double> dFstar;     // [NEI_SPAD]: their minima
    DevBuf<double> dZt;        // 2 x [Npad, NEI_SPAD]: Z and E transposed, of the call in progress
    DevBuf<double> dR, dG;     // 128 x Npad each: the running right-hand side / the solves' workspace
    DevBuf<int> dFlag;         // the X comparison's word
    DevBuf<double> dTab;       // [S, M]: the means of the table
    DevBuf<double> dPart;      // ... and the product's partial sums (paths_table_part_elems)
    DevBuf<double> dRowsPart;  // gp_nei_rows: the workgroups' shares (nei_rows_part_elems)
    DevBuf<double> dState;     // gp_nei_rows: ROWS_WIDE_M state rows of KG_STATE_STRIDE doubles
    int pass_launches = 0, pass_reads = 0;   // kernels the last pass of the last gp_nei_rows call put on the stream, and how many of them
                                             // read the inverse factor (0, 0: the call took the table route); counted where they are launched
};

// GP classification (api_laplace.hip): what a Laplace fit keeps beside the context's own buffers.  `on` while the context is
// "Laplace-fitted": dA holds the factor of K + W^-1, dAlpha the mode's a, and noise is 1 (noise_saved: what gp_set_params gave,
// put back where the state is dropped).  Every regression fit, gp_set_data and gp_set_params drop it (laplace_dropped).
enum { LAP_Y = 0, LAP_A, LAP_F, LAP_DA, LAP_DF, LAP_W, LAP_SW, LAP_B, LAP_T, LAP_RHS, LAP_SOL, LAP_S2, LAP_TMP, LAP_AU, LAP_U, LAP_NVEC };
struct LapState {
    bool on = false;
    double noise_saved = 0.0;
    DevBuf<double> dK;         // Npad x Npad: the full K of the fit in progress (no noise, no 1e-8), built once per call
    DevBuf<double> dVec;       // LAP_NVEC vectors of Npad (LAP_AU and LAP_U adjacent: the gradient pass's two rows a, u)
    DevBuf<double> dRes;       // LAP_RES_DOUBLES: the step's result block
    int iters = 0, halvings = 0;   // of the last fit (gp_laplace_info)
    double wmin = 0.0, wmax = 0.0;
};

struct gp_ctx {
    int device = 0;
    long lds_per_wg = 0;           // hipDeviceAttributeMaxSharedMemoryPerBlock of the device (gp_create)
    hipStream_t s = nullptr;       // main stream
    hipStream_t s_panel = nullptr; // look-ahead (panel chain) stream: high priority, all CUs
    hipStream_t s_bulk = nullptr;  // trailing-update stream of the look-ahead Cholesky: masked off the reserved CUs
    int bulk_reserved = -1;        // reserved-CU count s_bulk was created with
    hipStream_t s_inv = nullptr, s_pred = nullptr;  // pipelined candidate solve (gp_fit_predict), low priority
    // stream-ordering events of the look-ahead factorisation, one dense vector per role (EV_* below)
    std::vector<hipEvent_t> la_events[6];
    bool ev_error = false;         // a stream-ordering event could not be created (la_event); checked by la_events_ok
    // data: the seven buffers of gp_set_data share the capacity (capN rows, capP right-hand sides) and reallocate together
    long N = 0, Npad = 0;
    int D = 0, P = 0;
    DevBuf<double> dX, dY;
    DevBuf<double> dA;     // (Npad + 128) x Npad: Ky / L (lower) and, below it, the RHS rows (Y^T -> z^T)
    DevBuf<double> dInvL;  // nt tiles of 128 x 128: inverted diagonal tiles of L
    DevBuf<double> dAlpha; // P x Npad
    DevBuf<double> dW;     // P x Npad workspace
    DevBuf<double> dMu;    // (1 + TM_SPLIT) * N : training mean + partials
    DevBuf<int> dInfo;
    DevBuf<double> dScal;  // small scalars (scratch map above: SCAL_*)
    DevBuf<double> dRedV;  // reduction scratch, values (RED_*, REDV_*)
    DevBuf<long long> dRedI;   // ... and rows (RED_*, REDI_*)
    long capN = 0;
    int capP = 0;
    // params
    KernParams kp{};
    int ard = 0;
    double noise = 0.0;
    bool have_data = false, have_params = false;
    double jitter = 0.0, lml = 0.0, logdet = 0.0;
    double fmin = 0.0;
    // What the buffers hold.  A new factor in dA drops every one of these (factor_results_dropped, fit_dropped below); between
    // factors each is set where its buffer is filled and cleared where the buffer is reused for something else.
    bool fitted = false;       // dA holds L of the current data and parameters, dAlpha its alpha, lml / logdet / jitter belong to it
    bool fmin_valid = false;   // fmin is min over the training mean of the current fit
    bool wi_valid = false;     // dWi holds Ky^-1 of the factor
    bool li_valid = false;     // dLi holds L^-1 of the factor
    long rows_calls_since_fit = 0;   // *_rows calls that wanted the inverse factor since the last fit (build policy, api_rows.hip)
    bool w_in_t2 = false;      // dT2 still holds W = L^-T of the current factor (ensure_linv / ensure_wi)
    bool invp_valid = false;   // dInvP holds the inverted diagonal panels of the factor, invp_W tiles wide
    bool lr_valid = false;     // dLr belongs to the current factor
    bool predicted = false;    // dMean / dVar hold the posterior of the resident candidates (noise as predicted_noise), dT / dT2 what its solve left
    int cost_tab = 0;          // cost.dTabLogc holds logc of: 0 nothing, 1 the candidates in dXs, 2 the sparse model's table (sp.dTab);
                               // dropped where either table or the surface changes (gp_set_candidates*, gp_sparse_set_candidates, gp_cost_set)
    // candidates
    long M = 0;
    DevBuf<double> dXs;
    DevBuf<double> dT;     // Mc_pad x Npad
    DevBuf<double> dMean, dVar, dAcq;   // one capacity: the three reallocate together (ensure_out)
    int predicted_noise = -1;
    DevBuf<double> dWi;
    DevBuf<double> dT2;    // solved candidate rows S = K(Xs,X) L^-T (the running right-hand side stays in dT)
    // the explicit inverse factor and the scratch of the fused one-row path (onerow.hip, api_rows.hip)
    DevBuf<double> dLi;    // L^-1, lower triangular, Npad x Npad row-major, zeros above the diagonal
    DevBuf<double> dRows;  // RowsWork partials
    PassOwner pass{1, "the one-location kernels"};   // completion of the fused path's passes
    std::vector<double> lp_cache;       // local-penalisation batch as last uploaded (Xb | r | s), skipped when unchanged
    int lp_cache_nb = -1;
    long rows_fused_calls = 0, rows_fallback_calls = 0;
    long rows_narrow_passes = 0, rows_wide_passes = 0;   // fused passes of at most ROWS_MAX_M locations / of 5 .. ROWS_WIDE_M (gp_rows_pass_stats)
    int rows_wide = 1;                   // 5 .. 8 locations in ONE pass over the inverse factor (option "rows_wide"; 0: passes of four)
    int rows_build = -1;                 // inverse factor of the one-location path: -1 by the rule of api_rows.hip, 0 never, 1 at the first call (option "rows_build")
    int rows_nt = -1;                    // fused one-row path: non-temporal loads of the inverse factor (option "rows_nt"; -1: when its
                                         // lower triangle exceeds the 256 MiB Infinity Cache, N > 8192 -- measured -10 % at N = 16384,
                                         // +10 % at N = 4096 where the next call finds the factor cached: profiles/r05_small_calls.txt)
    DevBuf<double> dLp;    // local-penalisation batch: centres, radii, scales (LP_*)
    DevBuf<double> dApp;   // gp_append (api_append.hip): the border's scratch -- nothing in it outlives the call
    long append_in_place = 0, append_relayout = 0, append_refused = 0;   // borders written inside the last tile / into a new tile, calls refused (gp_append_stats)
    DevBuf<double> dX2, dK2;  // gp_cross_kernel_matrix: second input set and K(X, X2)
    DevBuf<double> dCov;   // full covariance / beta scratch
    DevBuf<double> dInvP, dInvPw;  // inverted diagonal panels L_JJ^-1 (+ build workspace)
    int invp_W = 0;
    DevBuf<double> dDm, dDv, dDacq;   // one capacity: the three reallocate together (ensure_grad_buffers)
    // options
    int panel_tiles = 6;
    int lookahead = 1;
    int inner_min_rows = 0;         // ... only while at least this many row tiles lie below the pair (below that the 128-column step's shorter launches win)
    // look-ahead factorisation, columns owned by the chain stream (factor_lookahead): the bulk stream keeps own_keep_base + own_keep_per_row * n
    // tiles of a trailing update with n row tiles below the look-ahead panel -- what lasts as long as the chain is busy with that panel --
    // and the rest, the far columns, is updated on the chain stream once the panel is done (every CU).  own_keep_per_row = 0: off.
    // Defaults from the sweep of round 4 (N = 8192 ... 32768, profiles/r04_own_columns.txt)
    int own_keep_per_row = 36, own_keep_base = 200;
    int own_keep_pipe_pct = 0;      // ... scaled by this while pipelined candidate stages share the bulk stream's CUs (0: the owned range stops shrinking there; fused step -0.3 ms)
    int inner_tiles = 1;            // tile columns per step of the in-panel factorisation (2: potrf_pair_kernel + trsm2 + K = 256 update;
                                    // measured in round 4: the same wall time as 1 at every size, profiles/r04_pair_step_experiment.txt)
    int lookahead_min_tiles = 40;   // gp_fit: matrices of at most this many tiles (N <= 5120) take the single-stream factorisation
    int reserve_cus = 32;
    long mc_max = 16384;
    long small_m = 8;        // up to this many candidates take the matrix-vector solve (smallm.hip) instead of the tile path
    // profiling
    Phase phases[MAX_PHASES];
    int nphases = 0;
    bool profiling = false;
    int profile_class = 0;   // which kernel symbol gp_profile brackets: 0 = the 8-wave 128-tile update, 1 = the 64 x 64 work-unit update
    std::vector<hipEvent_t> gemm_events;
    std::vector<hipEvent_t> rns_events;   // gp_profile: start / end of every residue GEMM launch (rns_gemm256_kernel)
    size_t rns_ev_used = 0;
    double rns_ops = 0.0;                 // int8 multiply-adds x 2 of those launches
    std::vector<long> gemm_tiles;
    std::map<std::array<int, 5>, DevBuf<short>> tile_lists;  // cached L2-friendly tile orders (device)
    int supertile = 8;  // long rectangular / triangular launches walk 8 x 8 super-tiles per XCD (fabric traffic 5.35 -> 3.72 GB per launch, same time)
    int small_below = 1400;  // launches with fewer 128-tiles than this use 64x64 workgroup tiles
    int chain_small_below = 400;  // ... the same threshold for the launches of the factorisation's chain stream
    int lauum_panels = 1;    // Ky^-1 product accumulated per k-panel (0: one launch over the whole contraction)
    int side_alpha = 1;      // alpha / log det on the side stream while stages of the one-call entry points still run
    int pair_panels = 1;     // candidate solve: two panels per update launch (K = 2 x panel width), bitwise the same result
    int pair_tri = 2;        // triangular-K products: pair column tiles c and W-1-c in one workgroup (1: 64x64 units only)
    int fmin_direct = 0;     // gp_fmin through the N^2 product K(X,X) alpha instead of y - d alpha
    int trsm_rows64 = 32;    // in-place panel solves as 64- or 32-row strips of the tile (2 or 4 workgroups per tile)
    int waves8 = 1;
    int stagger = 3;  // see gemm.hip: odd-slot workgroups start 3 * 1024 cycles late (+1.5 % measured)
    int gemm_sched = 1;       // the 8-wave instance with the scheduled K loop (gemm_nt_sched_kernel); 0: the plain loop.  The same bits
    int gemm_sched_side = 0;  // ... also on the side streams of the look-ahead factorisation (gemm() says why not)
    int long_min_tiles = 1024;  // launches of at least this many 128-tiles are "long": 8-wave instance, stagger (tests lower it)
    int pipe_stages_grad = 0, pipe_start_pct_grad = 40;  // the same for gp_fit_grad (stages of the solve for L^-T)
    int pipe_stages = 0;         // gp_fit_predict: candidate stages that ride behind the factorisation (rest afterwards)
    int pipe_done = 0;           // ... how many did, in the last factorisation
    int pipe_start_pct = -1;     // ... released once this share of the panels is factored (the chain sets the pace from there); -1: 32 % up to 24 panels, 40 % beyond (measured N = 8192 ... 32768)
    std::vector<int> gemm_K;
    size_t gemm_ev_used = 0;
    long gemm_launches = 0;
    double gemm_flops = 0.0;      // flops of the event-bracketed launches
    double gemm_flops_all = 0.0;  // flops of every GEMM launch since gp_profile(1)
    long profile_min_tiles = 1024;
    // comm
    ncclComm_t comm = nullptr;
    int rank = 0, nranks = 1;
    DevBuf<double> dComm;  // local top-k and gather scratch of the exchanges (COMM_*)
    // fp64 emulation on the int8 matrix cores (rns.hip)
    int emulate_fp64 = 0;
    int rns_group = 8; // panels per residue launch of the emulated candidate solve
    int rns_group_fit = 8;  // ... and of the emulated trailing update of the factorisation
    DevBuf<signed char> dLr, dSr, dRr;  // residue planes of L, of the current S panel, accumulator
    DevBuf<signed char> dRm;            // residue accumulator of the trailing matrix (factorisation)
    DevBuf<signed char> dWr;            // residue planes of W = L^-T (emulated Ky^-1)
    std::vector<char> lr_done;      // dLr, per panel: rows below the panel's diagonal block converted
    int lr_W = 0, lr_e = 0;
    double jitter_try = 0.0;        // jitter of the factorisation attempt in progress (fixes the fixed-point scale)
    int emulate_fit = 1;            // emulate_fp64 also covers the factorisation's trailing update
    bool emu_off_call = false;      // this call fell back to true fp64 (an operand left the fixed-point range)
    long emu_fallbacks = 0;         // how often that happened
    // gp_fit_grad_batch (api_batch.hip): buffers of its own, sized to the R and Npad in use -- never the resident fit's
    DevBuf<double> dBatch;
    DevBuf<signed char> dBatchAux;   // per-member KernParams table, then factorisation status words
    // gp_sparse_fit_grad_batch (api_sparse_batch.hip): buffers of its own, sized to the R, Mz and Npad in use -- never the
    // resident sparse fit's, the sparse candidate table's or the exact batch's
    DevBuf<double> dSpBatch;
    DevBuf<signed char> dSpBatchAux;   // per-member KernParams table, then factorisation status words
    // output warp (api_warp.hip): warp.n > 0 while one is on -- dY then holds f(dYraw), dYraw the targets gp_set_data brought
    WarpParams warp{0, 1.0, {}, {}, {}};
    DevBuf<double> dYraw;  // N: the raw targets of a warped model
    double warp_logjac = 0.0;   // sum log f'(y) of the warp in force
    DevBuf<double> dWarp;  // 9 M: posterior by value (mean, var), then warped mean, variance, median and the four partials
    SparseState sp;     // the sparse model (api_sparse.hip)
    EnsState ens;       // the ensemble (api_ens.hip)
    EsState es;         // entropy search: representers and belief (api_es.hip)
    CostState cost;     // the cost surface of the flagged scoring calls (api_cost.hip)
    MeanState mean;     // the mean function (api_mean.hip)
    FeasState feas;     // the cached probability of feasibility of the flagged table entries (api_feas.hip)
    EhviState ehvi;     // the cell decomposition behind the expected hypervolume improvement (api_ehvi.hip)
    MesState mes;       // the samples of the minimum's value behind GP_ACQ_MES (api_mes.hip)
    PathsState paths;   // posterior function samples over the resident factor (api_paths.hip)
    QeiState qei;       // the base samples of the joint expected improvement (api_qei.hip)
    KgState kg;         // the knowledge gradient's discretisation points (api_kg.hip)
    LapState lap;       // GP classification: the Laplace fit's buffers and state (api_laplace.hip)
    NeiState nei;       // noisy expected improvement: the fantasies this context holds as a twin (api_nei.hip)
    long linv_builds = 0;             // how often ensure_linv built the inverse factor since the context was created (gp_nei_stats)
    unsigned long long fit_gen = 0;   // a process-wide serial taken whenever the factor is dropped or grows: what gp_nei_set records of its model
    bool dead = false;  // gp_shutdown ran: the device's streams are gone, only gp_destroy is still valid
};

// The context stops being Laplace-fitted: the noise gp_set_params gave is in force again.  (Before anything reads g->noise for a
// regression fit, and before gp_set_params stores a new one.)
static inline void laplace_dropped(gp_ctx *g) {
    if (!g->lap.on) return;
    g->lap.on = false;
    g->noise = g->lap.noise_saved;
}
// The entries that read more of a fit than its factor, inverse factor, alpha and noise -- targets, log-likelihood pieces, the
// Gaussian LML's weights -- would answer silently wrong on a Laplace-fitted context: refused before anything is launched or changed
#define GP_NO_LAPLACE(g, who)                                                                       \
    do {                                                                                            \
        if ((g)->lap.on)                                                                            \
            return fail(GP_ERR_STATE, "%s: not available on a Laplace-fitted handle (gp_laplace_fit): a regression fit, gp_set_data or gp_set_params clears that state", who); \
    } while (0)

unsigned long long next_fit_gen();   // api_core.hip: 1, 2, ... over the process, never repeated
bool ctx_alive(gp_ctx *g);           // api_core.hip: g was created and not yet destroyed
// api_core.hip: g is a live context whose fit is current and has generation `gen` -- looked up and read under the lock gp_destroy
// takes before it frees a context, so a model destroyed on another thread is never dereferenced
bool ctx_fit_is(gp_ctx *g, unsigned long long gen);

// A new factor is about to be (or has been) written to dA: nothing derived from the old one may be served again.
static inline void factor_results_dropped(gp_ctx *g) {
    g->fit_gen = next_fit_gen();
    g->nei.S = 0;
    g->wi_valid = false;
    g->li_valid = false;
    g->rows_calls_since_fit = 0;
    g->w_in_t2 = false;
    g->invp_valid = false;
    g->lr_valid = false;
    g->predicted = false;
    g->es.R = 0;
    g->es.belief = false;
    g->kg.A = 0;
    g->paths.S = 0;
}
// ... and dA no longer holds a fit of the current data and parameters at all.
static inline void fit_dropped(gp_ctx *g) {
    laplace_dropped(g);
    factor_results_dropped(g);
    g->fitted = false;
    g->fmin_valid = false;
}

// the sparse fit no longer belongs to the data / parameters / inducing inputs in force, and neither does the cached posterior of
// the sparse candidate table (the table itself stays, as Z does), nor G of the second point set (the points stay too)
static inline void sparse_fit_dropped(gp_ctx *g) {
    g->sp.fitted = g->sp.grad_ready = g->sp.tab_post = g->sp.tab_grad = g->sp.fmin_valid = g->sp.zs_valid = g->sp.g_valid = false;
}

// The factor in dA has GROWN by rows (gp_append): L, the inverted diagonal tiles and -- where it was valid -- the inverse factor
// were extended and stay; rows_calls_since_fit keeps counting towards the inverse factor's build.  Everything else derived from
// the old factor or the old data is dropped, as gp_set_data drops it.
static inline void factor_grown(gp_ctx *g) {
    g->fit_gen = next_fit_gen();
    g->nei.S = 0;
    g->wi_valid = false;
    g->w_in_t2 = false;
    g->invp_valid = false;
    g->lr_valid = false;
    g->predicted = false;
    g->fmin_valid = false;
    sparse_fit_dropped(g);
    g->ens.S = 0;
    g->es.R = 0;
    g->es.belief = false;
    g->kg.A = 0;
    g->paths.S = 0;
}

static inline long round_up(long x, long m) { return (x + m - 1) / m * m; }

// The pass loop of the three fused rows paths: `width` locations per pass, each pass with a ticket and counter bases of its own
// from `own`.  launch(rx, r, arrivals) puts a pass on the stream and says how many arrivals its counters take (arrivals[1]: the
// ensemble's members), or returns an error; unpack(m0, mc, block) takes the results of locations [m0, m0 + mc) out of the pinned
// block.  A template over the two callables, inlined: no std::function and no allocation on a ~40 us call.
template <class Launch, class Unpack>
static inline int rows_passes(gp_ctx *g, PassOwner &own, const double *Xs, int M, int width, Launch launch, Unpack unpack) {
    const int D = g->D;
    for (int m0 = 0; m0 < M; m0 += width) {
        const int mc = std::min(width, M - m0);
        RowsX rx;
        rx.M = mc;
        memcpy(rx.xs, Xs + (long)m0 * D, sizeof(double) * mc * D);
        const PassReport r = own.next();
        unsigned arrivals[2] = {0, 0};
        int rc;
        if ((rc = launch(rx, r, arrivals))) return rc;
        if ((rc = own.wait(g->s, r, arrivals[0], arrivals[1]))) return rc;
        unpack(m0, mc, own.block);
    }
    return 0;
}
// Locations [m0, m0 + mc) of a call out of a block laid out for MV locations -- [mean][var][acq][dmdx][dvdx][dacq], gphip_internal.h
// -- into the caller's mean / var / acq [M] and dmdx / dvdx / dacq [M, D] (any may be null).
static inline void rows_unpack(const double *o, int MV, int m0, int mc, int D, double *mean, double *var, double *acq, double *dmdx,
                               double *dvdx, double *dacq) {
    for (int m = 0; m < mc; ++m) {
        if (mean) mean[m0 + m] = o[m];
        if (var) var[m0 + m] = o[MV + m];
        if (acq) acq[m0 + m] = o[2 * MV + m];
        const double *gm = o + 3 * MV + (long)m * D, *gv = gm + (long)MV * D, *ga = gv + (long)MV * D;
        if (dmdx) memcpy(dmdx + (long)(m0 + m) * D, gm, sizeof(double) * D);
        if (dvdx) memcpy(dvdx + (long)(m0 + m) * D, gv, sizeof(double) * D);
        if (dacq) memcpy(dacq + (long)(m0 + m) * D, ga, sizeof(double) * D);
    }
}

// the factorisation's trailing update runs in residue form (option emulate_fp64 with emulate_fit; panel edges on 256-column blocks)
static inline bool emu_fit_applies(const gp_ctx *g) {
    const long PB = (long)g->panel_tiles * GP_TILE;
    return g->emulate_fp64 && g->emulate_fit && !g->emu_off_call && (PB % 256 == 0) && PB <= GP_RNS_KMAX;
}

static inline GemmOpt inplace_opt() {
    GemmOpt o;
    o.inplace = 1;
    return o;
}

// ---- members ------------------------------------------------------------------------------------------------------------
// Where the operands of the single-stream fit-and-gradient sequences live, and how many independent problems ("members": the
// context's shapes, each with hyper-parameters of its own) ride side by side in every launch.  Member z's operand is
// at base + z * stride, its inputs and targets included: stride 0 where the members share the context's X or Y
// (gp_fit_grad_batch), a stride where each has its own (the warped models' batches, api_batch.hip).  The context's own fit is ONE
// member over its buffers (ctx_members, strides unused); the batch entries pass nb members over g->dBatch.  The sequences below are written once over this description; which kernel a launch of one
// or of several members runs is the launchers' business (gphip_internal.h) and gemm()'s.
struct Members {
    int nb = 1;
    long sA = 0, sI = 0, sP = 0, sV = 0, sT = 0, sS = 0;   // per-member strides (doubles) of the operand groups below, in their order
    const double *X = nullptr, *Y = nullptr;   // inputs [N, D] and targets [N, P], row-major
    long sX = 0, sY = 0;                       // ... and their per-member strides (0: shared)
    double *A = nullptr;      // Ky / L (lower) and, below it, the RHS rows: leading dimension lda
    long lda = 0;
    double *invL = nullptr;   // inverted diagonal tiles
    double *invP = nullptr, *invPw = nullptr;   // inverted diagonal panels of W tiles and their build workspace
    int W = 0;
    double *alpha = nullptr, *w = nullptr;      // P x Npad each
    // Npad x Npad each: the identity / running right-hand side, L^-T, Ky^-1 (may be T again) and the gradient pass's per-tile
    // partials (any of them that is free by then)
    double *T = nullptr, *T2 = nullptr, *Wi = nullptr, *partial = nullptr;
    double *scal = nullptr;   // SCAL_LOGDET, SCAL_DOT and SCAL_GRAD of the scratch map
    int *info = nullptr;      // 4 status words per member
    // per-member values: on the host (nb entries; a launch of one member passes them in its kernel arguments) and the same
    // in device tables (launches of several members index them; unused, and may be null, for one member)
    const KernParams *kp = nullptr, *kpt = nullptr;
    const double *diag = nullptr, *diag_tab = nullptr;   // what the diagonal of K gets: noise + 1e-8
    const double *jit = nullptr, *jit_tab = nullptr;     // the jitter of the attempt in progress
};
Members ctx_members(gp_ctx *g);                          // api_core.hip: the context's buffers as they are NOW (take it at the point of use)
Members members_range(const Members &m, int m0, int nb); // members [m0, m0 + nb) of m
// the GEMM options of a launch over m's members: per-member strides of C, A and B
static inline GemmOpt member_opt(const Members &m, GemmOpt o, long sC, long sA, long sB) {
    o.batch = o.members = m.nb;
    o.sC = sC;
    o.sA = sA;
    o.sB = sB;
    return o;
}
// The front end the batched entries share (api_batch.hip).
// member_params: variance[r], noise[r] and member r's lengthscale(s) are positive (GP_ERR_ARG names the member), then kp[r] = the
// context's kernel, dimension and Gower set-up with member r's variance and lengthscale(s).  Host only: nothing is reserved or
// launched.
int member_params(const gp_ctx *g, int nb, const double *variance, const double *lengthscale, const double *noise,
                  std::vector<KernParams> *kp);
// batch_members: kp.size() exact-model members over g->dBatch / g->dBatchAux -- the strides, every operand group of *m with the
// members side by side, the parameter, diagonal and jitter tables (m->kpt, diag_tab, jit_tab; *dJit the last, to write), m->info
// behind the parameter table.  On g->s: m->invL is zeroed, kp and diag (m->kp, m->diag: they outlive m) go to their tables.
// Behind the members the caller's own `extra` doubles from *extra_at on and, behind the (then 256-byte padded) info words, its
// `aux_extra` bytes at *aux_at (may be null without any).  m->jit, X and Y are the caller's.
int batch_members(gp_ctx *g, const std::vector<KernParams> &kp, const std::vector<double> &diag, long extra, size_t aux_extra,
                  Members *m, double **dJit, double **extra_at, signed char **aux_at);
// members_ladder: one jitter ladder (GPy/GPy/util/linalg.py:56-81) per member of m, those with active[r] set, factored in place
// in the members' A with nt tile columns and one RHS tile row below.  A round: for each run of consecutive active members,
// build(run, m0, jittered) writes everything the factorisation reads (the jitter of the attempt, jit[r] -- m.jit on the host, in
// dJit = m.jit_tab when given -- and the RHS rows included), the run's status words are cleared and factor_buf runs; then one
// copy of the status words and one synchronisation, and ladder_step per failed member: a failed member is factored again with the
// next jitter, alone with the other failed members, the others keep their factor.  diag0(failed, d0) is called once, after the
// first round when members failed, and fills d0[r], the mean diagonal the ladder starts from, for them.  Leaves st[r] (0, or the
// code the single call ends with) and jit[r] (the jitter of the member's last attempt); `active` is consumed.
// Deliberately NOT callers: fit_impl's ladder (api_factor.hip) and the posterior covariance's (api_predict.hip), which wrap the
// look-ahead scheduler with its pipes and a covariance that is not a Members problem.
using MembersBuild = std::function<int(const Members &run, int m0, bool jittered)>;
using MembersDiag0 = std::function<int(const std::vector<int> &failed, std::vector<double> &d0)>;
int members_ladder(gp_ctx *g, const Members &m, int nt, int maxtries, std::vector<int> &active, std::vector<double> &jit, double *dJit,
                   std::vector<int> &st, const MembersBuild &build, const MembersDiag0 &diag0);
// ... as the exact model's members take it: all of m's, Ky by build_ky, diag0[r] known beforehand (ky_diag)
int ky_ladder(gp_ctx *g, const Members &m, int maxtries, const std::vector<double> &diag0, std::vector<double> &jit, double *dJit,
              std::vector<int> &st);
// a member's non-zero status as the error of a call that one failed member fails
int ladder_failure(int st);

// Pipelined candidate solve (gp_fit_predict): as soon as panel J of L is final (chain(J) done), two more
// streams run, behind the factorisation and at low priority,
//   s_inv : invP_J = L_JJ^-1 (the per-panel build of ensure_panel_inv),
//   s_pred: S[:, J] = T[:, J] invP_J^T ;  T[:, > J] -= S[:, J] L[> J, J]^T
// so that the candidates' N^2 M flops fill the CUs the latency chain of the late panels leaves idle.
// (the solve runs on the context's dT / dT2 as T / S)
enum class Pipe { None, Candidates, Identity };   // what fit_impl pipelines: nothing, the resident candidates' solve, the identity's (L^-T, for Ky^-1)
struct PredPipe {
    bool on = false;
    int mt = 0;          // candidate row tiles
    int nJ = 0;          // panels of the factor
    std::function<void(hipStream_t)> init;  // fills T (cross covariance / identity) on the candidate stream, beside the factorisation's head
    bool trapezoid = false;  // T is block upper-triangular (the identity: the solve for L^-T), row tiles above the panel's end only
    int stages = 0, start_pct = 0;
    const char *phase = nullptr, *rest_phase = nullptr;   // profile phases: factorisation with the stages behind it, the stages after it
    double flops = 0.0;                                    // ... of the former
};

// The candidate solve S = T L^-T with the running right-hand side's updates  T[:, > J] -= S_J L[> J, J]^T  carried in
// residue form on the int8 matrix cores (rns.hip; option "emulate_fp64").  Per panel J: the fp64 columns of T are
// rebuilt from the exact integer accumulator, S_J = T_J invP_J^T runs in fp64 as before (5 % of the flops), S_J is
// converted to residues and ONE int8 launch (14 moduli) applies it to every column to the right.
// Shared state of the residue paths: fixed-point scale, residue planes of L (zeroed padding), per-panel conversion.
struct RnsGeom {
    int e = 0;
    double scale = 1.0, back = 1.0;
    long Lrows = 0, Lplane = 0, Lpitch = 0;   // row pitch of the residue planes of L in bytes (= Npad, api_rns.hip)
    int nt256 = 0;
};

// trapezoid (the solve of the identity, for Ky^-1): row tiles beyond a panel's end are still zero, so every step of panel J
// covers the row tiles [0, J1) only; the solved panels' residues are KEPT, all side by side in planes of N columns (Wr, for
// the product W W^T afterwards), and S = L^-T has its own fixed-point scale: its rows have norm sqrt((Ky^-1)_ii) <=
// 1 / sqrt(noise + 1e-8 + jitter), which takes the place of sqrt(max diag Ky) in the bound of rns.hip.
struct RnsSolveOpt {
    bool trapezoid = false;
    int eS = -1;                 // exponent of S's scale (2^(eS-1) >= the largest row norm of S); < 0: that of L
    signed char *Wr = nullptr;   // full residue planes of S: Wrows x wpitch bytes per plane, zero beyond the written rows
    long wpitch = 0, wplane = 0;
};

// One set of HIP streams per device for the whole process, created once in a fixed order and never destroyed.
// Hardware queues are dealt over the command processor's pipes in creation order, and two queues on one pipe do
// not overlap (a 6000-workgroup dispatch holds the pipe until its last workgroup is issued).  Measured: a context
// created after an earlier one was closed, or a re-created bulk stream, put the chain and the trailing update on
// one pipe and the factorisation went from 34 to 45 ms.  Order here: main, chain, bulk, inverse, candidates
// -> pipes 0,1,2,3,0.
struct DevStreams {
    hipStream_t s = nullptr, panel = nullptr, bulk = nullptr, inv = nullptr, pred = nullptr;
    int reserved = -1;
};

enum { EV_CHAIN = 0, EV_BULK = 1, EV_INVP = 2, EV_MISC = 3, EV_FAR = 4, EV_CONV = 5 };  // chain(J) done, bulk(J) done, invP_J built,
                                                                                    // fork/join/side, far launch of group g done, residues of panel J written

// ---- internal entry points (defined in the api_*.hip unit named in the comment of each group) ----
void shutdown_all();
int sparse_fitted(gp_ctx *g);   // api_sparse.hip: what every entry over a sparse fit asks first (alive, no mean function, data, parameters, Z, a fit)
int make_bulk_stream(int device, int reserve, hipStream_t *out);
int get_streams(int device, int reserve, DevStreams *out);
int phase_begin(gp_ctx *g, const char *name, double flops, double bytes);
void phase_end(gp_ctx *g, int id);
void gemm(gp_ctx *g, hipStream_t s, int mode, double *C, long ldc, const double *A, long lda, const double *B, long ldb, int b_mul, int K, TileSet ts, const GemmOpt &o = GemmOpt());
void rns_gemm(gp_ctx *g, hipStream_t s, const signed char *A, long lda, long a_plane, const signed char *B, long ldb, long b_plane, signed char *R, int mt_all, int nt_all, int mt, int c0, int c1, int K, int first, int tri = 0);
void destroy_ctx_events(gp_ctx *g);
void build_ky(gp_ctx *g, const Members &m, bool jittered);
void factor_buf(gp_ctx *g, const Members &m, int nt, int R1, bool side_inv = false);
int factor(gp_ctx *g);
void alpha_lml(gp_ctx *g, hipStream_t s, const Members &m);
void ky_diag(const KernParams &kp, double noise, double *diag_add, double *diag0);
int ladder_step(double diag0, int maxtries, int info, double *jitter, int *tries);
int factor_status(gp_ctx *g, bool emu, int *info, int *bad);
double lml_from_scalars(long N, int P, const double *scal);
void build_panel_inv_one(gp_ctx *g, hipStream_t s, int J, int W, int nt);
int rns_prepare(gp_ctx *g, double jitter, RnsGeom *r);
void rns_convert_panel(gp_ctx *g, hipStream_t s, const RnsGeom &r, int J, int *flag);
int factor_lookahead(gp_ctx *g, const PredPipe &pp = PredPipe());
int ensure_bulk_stream(gp_ctx *g);
hipEvent_t la_event(gp_ctx *g, int kind, size_t i);
int la_events_ok(gp_ctx *g);
int reserve_panel_inv(gp_ctx *g, int W, int nt);
int ensure_panel_inv(gp_ctx *g);
void identity_blocks(hipStream_t s, double *T, long n, int nb);
void panel_inv_members(gp_ctx *g, const Members &m);
void solve_step(gp_ctx *g, hipStream_t s, const Members &m, int J, int rows);
void solve_rows(gp_ctx *g, const Members &m, int mt, int trapezoid, int J_from = 0);
int solve_rows_rns(gp_ctx *g, double *T, double *S, int mt, const RnsSolveOpt &opt = RnsSolveOpt());
int fit_impl(gp_ctx *g, int maxtries, Pipe kind, int include_noise);
// chunk(m0, mc, mcpad), when given, runs after each chunk's reduce while dT2 still holds that chunk's solved rows (api_es.hip)
using ChunkHook = std::function<int(long, long, long)>;
int run_predict(gp_ctx *g, int include_noise, bool tiles_only = false, const ChunkHook *chunk = nullptr);   // tiles_only: never the small-M path (the caller uses dT2 as a padded tile operand)
int ensure_out(gp_ctx *g);
// What to score, as the C boundary got it: the base acquisition, and the local penaliser on top of it (the batch on the HOST)
// type: GP_ACQ_*, with GP_ACQ_PER_COST or-ed in when the scores are to be divided by the resident cost surface
// feas_ok: the entry understands GP_ACQ_TIMES_FEAS / GP_ACQ_POF (the exact table's value entries); everywhere else the bits stay
// in what acq_base returns and the call ends as an unknown acquisition
// mes_ok: the entry understands GP_ACQ_MES (the exact model's scoring entries, through exact_spec); everywhere else the rule is an
// unknown acquisition.  mes_y / mes_K: the context's resident samples on the device (exact_spec fills them in)
struct AcqSpec { int type; double par, fmin, y_mean, y_std; bool feas_ok = false; bool mes_ok = false; const double *mes_y = nullptr; int mes_K = 0; };
struct LpSpec { int transform; const double *Xb; int nb; const double *r0, *s0; };
static inline int acq_base(int type) { return type & ~GP_ACQ_PER_COST; }            // the acquisition itself
static inline bool acq_per_cost(int type) { return (type & GP_ACQ_PER_COST) != 0; }
static inline bool acq_times_feas(const AcqSpec &a) { return a.feas_ok && (a.type & GP_ACQ_TIMES_FEAS) != 0; }
static inline int acq_rule(const AcqSpec &a) { return acq_base(a.feas_ok ? a.type & ~GP_ACQ_TIMES_FEAS : a.type); }   // the rule a taught entry scores
// what an exact-model scoring entry hands on: a with GP_ACQ_MES understood and the resident samples attached (g may be null: the
// entry's own null check follows)
static inline AcqSpec exact_spec(const gp_ctx *g, AcqSpec a) {
    a.mes_ok = true;
    if (g) {
        a.mes_y = g->mes.dY.p;
        a.mes_K = g->mes.K;
    }
    return a;
}
// a single-output model, a known acquisition; with the flag: EI or MPI, a resident surface, no penaliser (lp null)
int check_acq(const gp_ctx *g, const AcqSpec &a, const LpSpec *lp = nullptr);
int check_per_cost(const gp_ctx *g, int type, bool lp);   // the flag's own conditions (no-op without it)
// api_cost.hip: the quotient behind the scores.  cost_divide: M rows at X on the device, acq [M] (and dacq [M, D] with grad) in
// place; a resident table (X == dXs or sp.dTab) pays the values' pass once per table and surface.  cost_divide_block: the
// locations of a fused rows pass, applied to its pinned result block (laid out for MV locations) behind the pass on the stream
int cost_divide(gp_ctx *g, const double *X, long M, bool grad, double *acq, double *dacq);
void cost_divide_block(gp_ctx *g, const RowsX &rx, bool grad, double *blk, int MV);
// api_feas.hip.  feas_apply: acq [M] of the resident candidates times exp of the cached log F (pof: -exp alone), on the stream
void feas_apply(gp_ctx *g, bool pof, double *acq);
// the table posterior of handle c over the locations already in its dXs: mean / var with noise and (grad) dDm / dDv, not drained
int table_posterior(gp_ctx *c, bool grad);
int train_values(gp_ctx *g);   // api_predict.hip: gp_fmin's quantity of every training row into dMu [N], not drained
// api_rows.hip: whether an M-location call of g takes the fused route now (counts towards the inverse factor's build policy), and
// one fused pass of g -- posterior, and the acquisition aq when on -- put on the stream WITHOUT the wait: *r is the pass's
// report, *arrivals what PassOwner::wait is owed.  The caller has several handles' passes of one device behind each other.
bool rows_take_fused(gp_ctx *g, int64_t M);
int rows_scratch(gp_ctx *g, RowsWork *w);   // the passes' partials over dRows, sized for a wide pass, and the owner made ready
int rows_prepare(gp_ctx *g);   // inverse factor, scratch, owner: everything that may synchronise, ahead of the first pass
void rows_enqueue(gp_ctx *g, const RowsX &rx, int include_noise, int want_grad, const RowsAcq &aq, PassReport *r, unsigned *arrivals);
int check_lp(const LpSpec &lp);                     // transform 0 / 1, 0 <= nb <= GP_LP_MAX_NB, a batch where nb > 0
int check_sense(int sense);
int check_k(int k);
int check_exclude(const int64_t *exclude, int nex, int64_t M);
// What every resident table (exact, sparse, ensemble, entropy search) scores, selects and hands over through (api_predict.hip)
int argbest_read(gp_ctx *g, const double *v, long n, int sense, int64_t *idx, double *val);   // lowest index among the best of v[0, n), drained
struct ScoreRows { const double *X; long M; const double *mean, *var, *dm, *dv; double *acq, *dacq; };   // M rows on the device and where their scores go
int score_rows(gp_ctx *g, const AcqSpec &a, const LpSpec *lp, bool grad, const ScoreRows &r);   // base acquisition (+ gradient), then the penaliser; no checks, no posterior
int select_best(gp_ctx *g, double *scores, long M, int sense, const int64_t *exclude, int nex, int64_t *idx, double *val);   // masks exclude [nex], then argbest_read
int select_topk(gp_ctx *g, double *scores, long M, int sense, int k, int64_t *idx, double *val);   // k rounds of arg-best + mask; the tail past M is -1 / acq_empty
int scores_out(gp_ctx *g, const double *acq, const double *dacq, long M, int D, double *out, double *dout);   // the drained copies (null: skipped)
static inline double acq_empty(int sense) { return sense > 0 ? -INFINITY : INFINITY; }   // the value no candidate loses to
struct LpBatch { double *X = nullptr, *r = nullptr, *s = nullptr; };   // the batch on the device
static inline LpBatch lp_slots(const gp_ctx *g) { return LpBatch{g->dLp + LP_X.off, g->dLp + LP_R.off, g->dLp + LP_S.off}; }
RowsAcq rows_acq(const AcqSpec &a, const LpSpec *lp, const LpBatch &b);   // the fused path's kernel argument (lp null: base only)
int run_acq(gp_ctx *g, const AcqSpec &a, const LpSpec *lp, bool grad);   // the exact table's scores into dAcq (dDacq with grad), checks and posterior included
int upload_lp_batch(gp_ctx *g, const LpSpec &lp, LpBatch *b);
int rows_lp_batch(gp_ctx *g, const LpSpec &lp, LpBatch *b);   // api_rows.hip: the same, skipped while dLp still holds this batch
int acq_values(gp_ctx *g, const AcqSpec &a, const LpSpec *lp, double *out, double *dout);   // api_grad.hip
// gp_acq_argbest / gp_acq_lp_argbest and gp_acq_topk over the specs, preamble included (lp null: no penaliser)
int acq_argbest(gp_ctx *g, const AcqSpec &a, const LpSpec *lp, int sense, const int64_t *exclude, int nex, int64_t *idx, double *val);
int acq_topk(gp_ctx *g, const AcqSpec &a, int sense, int k, int64_t *idx, double *val);
// {value, row} records of the gathers: n pairs of doubles, the second holding the row's 8 bytes (api_comm.hip)
void pack_pairs(const double *v, const int64_t *ix, size_t n, double *rec);
void unpack_pairs(const double *rec, size_t n, double *v, int64_t *ix);
void lauum(gp_ctx *g, const Members &m);
int wi_lauum(gp_ctx *g);
int wi_rns(gp_ctx *g);
int ensure_wi(gp_ctx *g);
int ensure_linv(gp_ctx *g);
// GP_ERR_ARG, with D, P, Gower, the bytes needed and the bytes there are, when a workgroup of launch_lml_grad / launch_gradx over
// the context's (D, Gower setting, P) needs more LDS than the device has; nothing is launched or changed.  `who`: the entry
int lml_grad_lds_check(const gp_ctx *g, const char *who);
int gradx_lds_check(const gp_ctx *g, const char *who);
void lml_grad_passes(gp_ctx *g, const Members &m);
void grads_from_sums(const double *h, const KernParams &kp, int ard, double *dvariance, double *dlengthscale, double *dnoise);
int lml_grad_impl(gp_ctx *g, double *dvariance, double *dlengthscale, double *dnoise, bool reset_phases, double *dL_dX = nullptr);
int ensure_grad_buffers(gp_ctx *g, long elemsBeta, long M);
int run_predict_grad(gp_ctx *g);
void panel_inv_steps(gp_ctx *g, hipStream_t s, double *Wb, long PB, const double *Lb, long lda, const double *Ib, int Wp, GemmOpt o,
                     long sL, long sI);   // api_solve.hip: Wb (the identity on entry) <- L^-T of the Wp-tile lower factor at Lb
// api_es.hip: what a scoring call needs -- an exact single-output model without a warp, representers and a belief --, and the
// pointers of the belief for a launch
int nei_ready(gp_ctx *g, double y_mean, double y_std, const char *who);   // api_nei.hip: resident fantasies of an unchanged model, a usable normaliser
int nei_table_scores(gp_ctx *g, double par, double y_mean, double y_std, const char *who);   // api_nei.hip: +NEI of the resident candidates into dAcq (not drained)
int kg_ready(gp_ctx *g, double y_std);   // api_kg.hip: an exact single-output model as KG takes it, resident points, a usable y_std
int es_ready(gp_ctx *g, double y_std);
struct EsBelief { const double *Qt, *Gt, *logP, *u, *W; };
EsBelief es_belief(const gp_ctx *g);
// api_mean.hip (each a no-op without a resident mean function): dY <- dYraw - m(X) where it is stale, enqueued and drained;
// mean [M, P] += m(X) for M rows X on the device; dmdx [M, D, P] += A; the fused rows passes' kernel argument
int mean_residuals(gp_ctx *g);
void mean_add(gp_ctx *g, const double *X, long M, double *mean);
void mean_add_grad(gp_ctx *g, long M, double *dmdx);
static inline RowsMean rows_mean(const gp_ctx *g) {
    return g->mean.on() ? RowsMean{1, g->mean.dAb.p, g->mean.dAb.p + (long)g->D * g->P} : RowsMean{0, nullptr, nullptr};
}
int warp_apply(gp_ctx *g, bool raw_in_dY);   // api_warp.hip: (dYraw <- dY when dY holds raw targets,) dY <- f(dYraw), warp_logjac; enqueued on g->s, the caller drains
