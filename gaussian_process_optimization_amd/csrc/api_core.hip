// Lifecycle of a context (gp_t), the per-device stream set, options, data / parameter upload, the accounted GEMM
// launcher and the small getters.  See include/gphip.h for the contract (reference file:line per entry point).
#include "api_internal.h"
#include <atomic>

#define BK_MIN 16  // the GEMM's stage depth (gemm.hip): every contraction length is a multiple of it

thread_local std::string g_err;

// first failed launch / stream operation of the calling thread since the last report (gphip_internal.h)
static thread_local bool g_note_set = false;
static thread_local std::string g_note_msg;

// Every error return of the library goes through here.  A launch failure noted earlier in the SAME call (GP_LAUNCH / GP_NOTE)
// that this return would otherwise leave behind -- the entry point is leaving before its GP_SYNC -- is folded into the message
// and cleared: it must not surface as the failure of the thread's next, unrelated call.
int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    if (g_note_set) {
        g_err += " [after: " + g_note_msg + "]";
        g_note_set = false;
    }
    return code;
}

void gp_note_hip(hipError_t e, const char *what, const char *file, int line) {
    if (e == hipSuccess || g_note_set) return;
    char buf[512];
    snprintf(buf, sizeof buf, "%s -> %s (%s:%d)", what, hipGetErrorString(e), file, line);
    g_note_msg = buf;
    g_note_set = true;
}
int gp_pending_error() {
    if (!g_note_set) return 0;
    g_note_set = false;
    return fail(GP_ERR_HIP, "%s", g_note_msg.c_str());
}
// A note that survived its call after all (an entry point that returned success without synchronising) is dropped when the next
// entry point starts: GP_DEAD_CHECK, the first thing every gp_* function does with its context.
void gp_clear_stale_note() { g_note_set = false; }

// ---- the completion of a fused rows pass (PassOwner, api_internal.h) ----
int PassOwner::make_ready(hipStream_t s) {
    int rc;
    if (!counter) {
        if ((rc = counter.reserve(words))) return rc;
        HIPCHK(hipMemsetAsync(counter, 0, sizeof(unsigned int) * words, s));
    }
    if (!block) {   // coherent host memory the finishing workgroup writes and the host reads after the sync
        HIPCHK(hipHostMalloc((void **)&block, sizeof(double) * (ROWS_OUT_DOUBLES + 1), hipHostMallocDefault));
        block[ROWS_OUT_DOUBLES] = 0.0;
    }
    return 0;
}
int PassOwner::restart(hipStream_t s) {
    if (!counter) return 0;
    HIPCHK(hipMemsetAsync(counter, 0, sizeof(unsigned int) * words, s));
    base[0] = base[1] = 0;
    return 0;
}
int PassOwner::wait(hipStream_t s, const PassReport &r, unsigned a0, unsigned a1) {
    base[0] += a0;
    base[1] += a1;
    hipError_t e = hipStreamSynchronize(s);
    int pending = gp_pending_error();
    if (!pending && e == hipSuccess && block[ROWS_OUT_DOUBLES] == r.ticket) return 0;
    // a launch did not complete and the counter may hold anything: cleared with the bases, so that the next call starts clean
    const std::string noted = pending ? gp_last_error() : std::string();
    hipStreamSynchronize(s);
    hipMemset(counter, 0, sizeof(unsigned int) * words);
    base[0] = base[1] = 0;
    if (pending) return fail(GP_ERR_HIP, "%s", noted.c_str());
    if (e != hipSuccess) return fail(GP_ERR_HIP, "hipStreamSynchronize -> %s (%s)", hipGetErrorString(e), who);
    return fail(GP_ERR_HIP, "%s did not complete (ticket %.0f, expected %.0f)", who, block[ROWS_OUT_DOUBLES], r.ticket);
}

static std::mutex g_ds_mu;
static std::map<int, DevStreams> g_ds;
static std::set<gp_ctx *> g_live;  // contexts created and not yet destroyed
static bool g_atexit_registered = false;

unsigned long long next_fit_gen() {
    static std::atomic<unsigned long long> gen{0};
    return ++gen;
}
bool ctx_fit_is(gp_ctx *g, unsigned long long gen) {
    std::lock_guard<std::mutex> lk(g_ds_mu);
    return g_live.count(g) != 0 && g->fitted && g->fit_gen == gen;
}
bool ctx_alive(gp_ctx *g) {
    std::lock_guard<std::mutex> lk(g_ds_mu);
    return g_live.count(g) != 0;
}

// Ordered shutdown (exported as gp_shutdown, and registered with atexit() at the first stream creation so that it runs
// BEFORE the HIP runtime's and a profiler's own exit handlers, which were registered earlier): quiesce every device the
// library touched, destroy the events recorded on the shared streams, then the streams.  Without it the five
// process-lifetime queues per device -- two of them created with hipExtStreamCreateWithCUMask -- were still alive when
// the runtime's static destructors ran; under rocprofv3 the runtime's queue teardown then called into the already
// finalised tool and the process died with SIGSEGV inside __cxa_finalize (round 1: every profiled run after the
// per-device stream set was introduced; plain runs exited 0).  See DESIGN.md, "Lifecycle".
void shutdown_all() {
    std::lock_guard<std::mutex> lk(g_ds_mu);
    for (auto &kv : g_ds) {
        if (hipSetDevice(kv.first) != hipSuccess) continue;
        hipDeviceSynchronize();
    }
    for (gp_ctx *g : g_live) {
        hipSetDevice(g->device);
        destroy_ctx_events(g);
        g->s = g->s_panel = g->s_bulk = g->s_inv = g->s_pred = nullptr;
        g->dead = true;
    }
    for (auto &kv : g_ds) {
        if (hipSetDevice(kv.first) != hipSuccess) continue;
        DevStreams &d = kv.second;
        for (hipStream_t *st : {&d.pred, &d.inv, &d.bulk, &d.panel, &d.s}) {
            if (*st) hipStreamDestroy(*st);
            *st = nullptr;
        }
    }
    g_ds.clear();
}
static void shutdown_atexit() { shutdown_all(); }

int make_bulk_stream(int device, int reserve, hipStream_t *out) {
    hipDeviceProp_t pr;
    HIPCHK(hipGetDeviceProperties(&pr, device));
    const int ncu = pr.multiProcessorCount;
    const int words = (ncu + 31) / 32;
    std::vector<uint32_t> mask(words, 0xffffffffu);
    // CU bits are dealt round-robin over the XCDs (measured: tools/micro/cumask.hip), so clearing the
    // lowest R bits reserves R/8 CUs on every XCD.
    for (int i = 0; i < reserve && i < ncu - 8; ++i) mask[i / 32] &= ~(1u << (i % 32));  // reserve may be large (half the chip)
    if (reserve > 0) {
        hipError_t e = hipExtStreamCreateWithCUMask(out, (uint32_t)words, mask.data());
        if (e != hipSuccess) return fail(GP_ERR_HIP, "hipExtStreamCreateWithCUMask -> %s", hipGetErrorString(e));
    } else {
        HIPCHK(hipStreamCreateWithFlags(out, hipStreamNonBlocking));
    }
    return 0;
}

int get_streams(int device, int reserve, DevStreams *out) {
    std::lock_guard<std::mutex> lk(g_ds_mu);
    if (const char *e = getenv("GPHIP_RESERVE_CUS")) reserve = std::max(0, std::min(64, atoi(e)));
    DevStreams &d = g_ds[device];
    if (!d.s) {
        if (!g_atexit_registered) {
            atexit(shutdown_atexit);
            g_atexit_registered = true;
        }
        int lo = 0, hi = 0;
        hipDeviceGetStreamPriorityRange(&lo, &hi);
        HIPCHK(hipStreamCreateWithPriority(&d.s, hipStreamNonBlocking, lo));
        HIPCHK(hipStreamCreateWithPriority(&d.panel, hipStreamNonBlocking, hi));
        int rc = make_bulk_stream(device, reserve, &d.bulk);
        if (rc) return rc;
        d.reserved = reserve;
        HIPCHK(hipStreamCreateWithPriority(&d.inv, hipStreamNonBlocking, lo));
        // the pipelined candidate solve launches thousands of workgroups too: keep it off the reserved CUs as well,
        // or the chain's diagonal-tile workgroup (which needs an EMPTY CU) waits for a whole candidate update
        {
            int rp = reserve;
            if (const char *e = getenv("GPHIP_PRED_RESERVE")) rp = atoi(e);
            rc = make_bulk_stream(device, rp, &d.pred);
            if (rc) return rc;
        }
    }
    // never re-created: the replacement queue lands on another command-processor pipe (creation order), and
    // when that is the chain stream's pipe the two can no longer overlap
    *out = d;
    return 0;
}

// ---- phase timing -----------------------------------------------------------------------------
int phase_begin(gp_ctx *g, const char *name, double flops, double bytes) {
    if (g->nphases >= MAX_PHASES) return -1;
    Phase &p = g->phases[g->nphases];
    p.name = name;
    p.flops = flops;
    p.bytes = bytes;
    if (!p.used) {
        hipEventCreate(&p.e0);
        hipEventCreate(&p.e1);
        p.used = true;
    }
    GP_NOTE(hipEventRecord(p.e0, g->s));
    return g->nphases++;
}
void phase_end(gp_ctx *g, int id) {
    if (id >= 0) GP_NOTE(hipEventRecord(g->phases[id].e1, g->s));
}

// ---- GEMM wrapper with accounting ---------------------------------------------------------------
// The instance is chosen from the tiles of ONE problem (n: a launch over several members gives each the instance it would get
// alone, and with it the same per-tile arithmetic); the accounting is that of the whole launch (n_all).  gp_profile brackets a
// launch over members when it would bracket one member's, and records the launch's tiles and flops.
void gemm(gp_ctx *g, hipStream_t s, int mode, double *C, long ldc, const double *A, long lda, const double *B, long ldb, int b_mul, int K, TileSet ts, const GemmOpt &o) {
    if (o.batch <= 0 || o.members <= 0) return;
    const long n = tileset_count(ts) * (o.batch / o.members), n_all = tileset_count(ts) * o.batch;
    if (n <= 0 || K <= 0) return;
    GemmOpt oo = o;
    if (n >= g->long_min_tiles && !oo.stagger) oo.stagger = g->stagger;
    if (n >= g->long_min_tiles && g->waves8) oo.waves8 = 1;  // 4 waves/SIMD: +2 % on the long launches (measured)
    // The scheduled K loop where a long launch has the chip to itself: on the context's own stream.  On the look-ahead's side
    // streams (trailing updates and pipelined candidate stages beside the factorisation's latency chain) each launch is faster
    // with it too, but the step is not: the chain, which sets the pace there, loses more than the launches gain (measured).
    oo.sched = g->gemm_sched && (s == g->s || g->gemm_sched_side);
    // ... or split each tile into two 64-row strips (a strip reads only its own rows of A: still safe in place)
    if (oo.inplace && g->trsm_rows64 && !oo.waves8) oo.rows64 = g->trsm_rows64;  // 1 / 64: two strips, 32: four
    // short launches (the factorisation's latency chain, the uneven triangular-K products) run as 64x64 work units
    const int small_thr = (s == g->s_panel) ? g->chain_small_below : g->small_below;
    if (small_thr > 0 && n < small_thr && !oo.inplace) oo.small = 1;
    // products with an inverted panel: column tile c contracts c+1 K-blocks; pairing c with W-1-c gives every
    // workgroup the same W+1 blocks (one balanced round of workgroups instead of a long and a short one)
    if (g->pair_tri && (oo.small || (oo.waves8 && g->pair_tri >= 2)) && o.k_end_tri && !ts.tri && !o.tile_list && ts.c1 - ts.c0 >= 2)
        oo.pair = 1;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    // events only around the launches that carry the flops (>= 1024 output tiles): bracketing every one of the
    // ~700 small launches of an iteration stalls the latency chain (34 -> 53 ms per factorisation, measured)
    // ... and only the launches of ONE kernel symbol, gemm_nt_kernel<1, 128, 4, false, 128> (C -= A B^T, 8 waves), so that the
    // average agrees with that symbol's row in a rocprofv3 --stats summary of the same command
    // gp_profile(2) brackets the OTHER fp64 symbol instead, gemm_nt_kernel<1, 64, 2, false, 64> (C -= A B^T as 64 x 64 work
    // units: the chain's in-panel / look-ahead updates and the short candidate updates) -- in a pass of its own, for the reason above
    const bool small_sym = mode == 1 && oo.small && !oo.pair && !oo.rows64;
    const bool timed = g->profiling && (g->profile_class == 1 ? small_sym :
                       (n >= g->profile_min_tiles &&
                        (g->profile_min_tiles < 1024 || (mode == 1 && oo.waves8 && !oo.small))));  // tracing tools lower the threshold
    if (timed) {
        if (g->gemm_ev_used + 2 > g->gemm_events.size()) {
            hipEvent_t a, b;
            hipEventCreate(&a);
            hipEventCreate(&b);
            g->gemm_events.push_back(a);
            g->gemm_events.push_back(b);
        }
        e0 = g->gemm_events[g->gemm_ev_used++];
        e1 = g->gemm_events[g->gemm_ev_used++];
        GP_NOTE(hipEventRecord(e0, s));
        g->gemm_tiles.push_back(n_all);
        g->gemm_K.push_back((o.k_tri || o.k_end_tri) ? -K : K);
    }
    if (g->supertile > 1 && !o.tile_list && !o.k_end_tri && o.batch == 1 && tileset_count(ts) >= 2048) {
        const std::array<int, 5> key{ts.r0, ts.r1, ts.c0, ts.c1, ts.tri};
        auto it = g->tile_lists.find(key);
        if (it == g->tile_lists.end()) {
            std::vector<short> l = build_tile_list(ts, g->supertile);
            DevBuf<short> d;
            if (d.alloc((long)l.size()) == hipSuccess) {   // (not reserve: a launch without its list is no error)
                hipMemcpy(d, l.data(), l.size() * sizeof(short), hipMemcpyHostToDevice);
                it = g->tile_lists.emplace(key, std::move(d)).first;
            }
        }
        if (it != g->tile_lists.end()) oo.tile_list = it->second;
    }
    launch_gemm_nt(s, mode, C, ldc, A, lda, B, ldb, b_mul, K, ts, oo);
    if (timed) {
        GP_NOTE(hipEventRecord(e1, s));
        g->gemm_launches++;
        g->gemm_flops += 2.0 * GP_TILE * GP_TILE * (double)K * (double)n_all * ((o.k_tri || o.k_end_tri) ? 0.5 : 1.0);
    }
    g->gemm_flops_all += 2.0 * GP_TILE * GP_TILE * (double)K * (double)n_all * ((o.k_tri || o.k_end_tri) ? 0.5 : 1.0);
}

// ---- members (api_internal.h) -------------------------------------------------------------------
Members ctx_members(gp_ctx *g) {
    Members m;
    m.A = g->dA;
    m.lda = g->Npad;
    m.invL = g->dInvL;
    m.info = g->dInfo;
    m.invP = g->dInvP;
    m.invPw = g->dInvPw;
    m.W = g->invp_W;
    m.alpha = g->dAlpha;
    m.w = g->dW;
    m.T = g->dT;
    m.T2 = g->dT2;
    m.Wi = g->dWi;
    m.partial = g->dT;   // free once Ky^-1 is in dWi
    m.scal = g->dScal;
    m.kp = &g->kp;
    m.X = g->dX;
    m.Y = g->dY;
    return m;
}

Members members_range(const Members &m, int m0, int nb) {
    Members r = m;
    r.nb = nb;
    r.A += m0 * m.sA;
    r.invL += m0 * m.sI;
    r.info += 4 * m0;
    r.scal += m0 * m.sS;
    r.X += m0 * m.sX;
    r.Y += m0 * m.sY;
    for (double **q : {&r.invP, &r.invPw}) *q += m0 * m.sP;
    for (double **q : {&r.alpha, &r.w}) *q += m0 * m.sV;
    for (double **q : {&r.T, &r.T2, &r.Wi, &r.partial}) *q += m0 * m.sT;
    for (const KernParams **q : {&r.kp, &r.kpt}) *q += m0;
    for (const double **q : {&r.diag, &r.diag_tab, &r.jit, &r.jit_tab}) *q += m0;
    return r;
}

extern "C" const char *gp_last_error(void) { return g_err.c_str(); }
extern "C" const char *gp_version(void) { return "gphip 0.1 (gfx950, fp64 MFMA)"; }

extern "C" int gp_device_count(int *count) {
    if (!count) return fail(GP_ERR_ARG, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(GP_ERR_HIP, "hipGetDeviceCount -> %s", hipGetErrorString(e));
    }
    *count = n;
    return 0;
}

extern "C" int gp_device_info(int device, char *name, int cap, int *cus, int64_t *hbm_bytes) {
    hipDeviceProp_t pr;
    HIPCHK(hipGetDeviceProperties(&pr, device));
    if (name && cap > 0) {
        snprintf(name, cap, "%s (%s)", pr.name, pr.gcnArchName);
    }
    if (cus) *cus = pr.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (int64_t)pr.totalGlobalMem;
    return 0;
}

extern "C" int gp_create(gp_t **out, int device) {
    if (!out) return fail(GP_ERR_ARG, "out is NULL");
    int n = 0;
    HIPCHK(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail(GP_ERR_ARG, "device %d out of range (%d visible)", device, n);
    HIPCHK(hipSetDevice(device));
    int lds = 0;   // what the gradient entries hold their staging against (lml_grad_lds_check)
    HIPCHK(hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
    gp_ctx *g = new gp_ctx();
    g->device = device;
    g->lds_per_wg = lds;
    for (int i = 0; i < MAX_PHASES; ++i) g->phases[i].used = false;
    {
        DevStreams d;
        int rcs = get_streams(device, g->reserve_cus, &d);
        if (rcs) {
            delete g;
            return rcs;
        }
        g->s = d.s;
        g->s_panel = d.panel;
        g->s_bulk = d.bulk;
        g->bulk_reserved = d.reserved;
        g->s_inv = d.inv;
        g->s_pred = d.pred;
    }
    int rc = g->dInfo.reserve(4);
    if (!rc) rc = g->dScal.reserve(SCAL_CAP);
    if (!rc) rc = g->dRedV.reserve(REDV_CAP);
    if (!rc) rc = g->dRedI.reserve(REDI_CAP);
    if (rc) {
        delete g;
        return rc;
    }
    {
        std::lock_guard<std::mutex> lk(g_ds_mu);
        g_live.insert(g);
    }
    // run an unmodified host program (e.g. the whole GPU test suite) with the emulated contractions on
    if (const char *ev = getenv("GPHIP_EMULATE_FP64")) g->emulate_fp64 = atoi(ev) ? 1 : 0;
    if (const char *ev = getenv("GPHIP_INNER_TILES")) g->inner_tiles = atoi(ev) == 2 ? 2 : 1;
    if (const char *ev = getenv("GPHIP_INNER_MIN_ROWS")) g->inner_min_rows = std::max(0, atoi(ev));   // A/B of the in-panel step across unmodified tools
    if (const char *ev = getenv("GPHIP_OWN_KEEP_PER_ROW")) g->own_keep_per_row = std::max(0, atoi(ev));
    if (const char *ev = getenv("GPHIP_OWN_KEEP_BASE")) g->own_keep_base = std::max(0, atoi(ev));   // (a wide owned range forced on an unmodified test suite)
    *out = g;
    return 0;
}

extern "C" int gp_shutdown(void) {
    shutdown_all();
    return 0;
}

void destroy_ctx_events(gp_ctx *g) {
    for (int i = 0; i < MAX_PHASES; ++i)
        if (g->phases[i].used) {
            hipEventDestroy(g->phases[i].e0);
            hipEventDestroy(g->phases[i].e1);
            g->phases[i].used = false;
        }
    g->nphases = 0;
    for (hipEvent_t e : g->gemm_events) hipEventDestroy(e);
    g->gemm_events.clear();
    for (hipEvent_t e : g->rns_events) hipEventDestroy(e);
    g->rns_events.clear();
    g->rns_ev_used = 0;
    g->gemm_ev_used = 0;
    g->gemm_tiles.clear();
    g->gemm_K.clear();
    for (auto &v : g->la_events) {
        for (hipEvent_t e : v)
            if (e) hipEventDestroy(e);
        v.clear();
    }
}

extern "C" int gp_destroy(gp_t *g) {
    if (!g) return 0;
    {
        std::lock_guard<std::mutex> lk(g_ds_mu);
        if (!g_live.erase(g)) return 0;  // not a live context (double destroy)
    }
    hipSetDevice(g->device);
    hipDeviceSynchronize();
    if (g->comm) ncclCommDestroy(g->comm);
    // events recorded on the shared streams go first; the streams themselves belong to the per-device set shared by
    // every context of the process and are destroyed by gp_shutdown / the exit hook
    destroy_ctx_events(g);
    delete g;   // every device buffer is freed by its DevBuf, the pinned result blocks by their PassOwner
    return 0;
}

// ---- options --------------------------------------------------------------------------------------
// The options that are one int of the context, and how each takes its value:
//   OPT_RANGE  stored when in [lo, hi], GP_ERR_ARG otherwise      OPT_BOOL  0 or 1
//   OPT_FLOOR  GP_ERR_ARG below lo, clamped to 1 << 20 above      OPT_RAW   as it is
// gp_set_option looks a name up here first; what an option does beyond the store follows the table there.
enum OptShape { OPT_RANGE, OPT_FLOOR, OPT_BOOL, OPT_RAW };
struct OptDesc {
    const char *name;
    int gp_ctx::*field;
    OptShape shape;
    int lo, hi;
};
static const OptDesc g_options[] = {
    {"panel_tiles", &gp_ctx::panel_tiles, OPT_RANGE, 1, 64},
    {"inner_tiles", &gp_ctx::inner_tiles, OPT_RANGE, 1, 2},
    {"inner_min_rows", &gp_ctx::inner_min_rows, OPT_FLOOR, 0},
    {"own_keep_per_row", &gp_ctx::own_keep_per_row, OPT_FLOOR, 0},
    {"own_keep_pipe_pct", &gp_ctx::own_keep_pipe_pct, OPT_RANGE, 0, 400},
    {"own_keep_base", &gp_ctx::own_keep_base, OPT_FLOOR, 0},
    {"lookahead", &gp_ctx::lookahead, OPT_BOOL},
    {"lookahead_min_tiles", &gp_ctx::lookahead_min_tiles, OPT_FLOOR, 0},
    {"pipe_start_pct", &gp_ctx::pipe_start_pct, OPT_RANGE, -1, 100},   // -1: automatic
    {"small_below", &gp_ctx::small_below, OPT_RAW},
    {"pipe_stages_grad", &gp_ctx::pipe_stages_grad, OPT_FLOOR, 0},
    {"pipe_start_pct_grad", &gp_ctx::pipe_start_pct_grad, OPT_RANGE, 0, 100},
    {"pipe_stages", &gp_ctx::pipe_stages, OPT_FLOOR, 0},
    {"lauum_panels", &gp_ctx::lauum_panels, OPT_RAW},
    {"side_alpha", &gp_ctx::side_alpha, OPT_RAW},
    {"pair_panels", &gp_ctx::pair_panels, OPT_BOOL},
    {"pair_tri", &gp_ctx::pair_tri, OPT_RAW},
    {"fmin_direct", &gp_ctx::fmin_direct, OPT_RAW},
    {"chain_small_below", &gp_ctx::chain_small_below, OPT_RAW},
    {"waves8", &gp_ctx::waves8, OPT_BOOL},
    {"stagger", &gp_ctx::stagger, OPT_RAW},
    {"gemm_sched", &gp_ctx::gemm_sched, OPT_BOOL},
    {"gemm_sched_side", &gp_ctx::gemm_sched_side, OPT_BOOL},
    {"long_min_tiles", &gp_ctx::long_min_tiles, OPT_FLOOR, 1},
    {"trsm_rows64", &gp_ctx::trsm_rows64, OPT_RAW},
    {"rns_group_fit", &gp_ctx::rns_group_fit, OPT_RANGE, 1, 16},
    {"rns_group", &gp_ctx::rns_group, OPT_RANGE, 1, 16},
    {"emulate_fit", &gp_ctx::emulate_fit, OPT_BOOL},
    {"emulate_fp64", &gp_ctx::emulate_fp64, OPT_BOOL},
    {"rows_build", &gp_ctx::rows_build, OPT_RANGE, -1, 1},   // -1: by rule, 0: never, 1: at the first call
    {"rows_nt", &gp_ctx::rows_nt, OPT_RANGE, -1, 1},         // -1: automatic
    {"rows_wide", &gp_ctx::rows_wide, OPT_BOOL},             // 5 .. 8 locations in one pass (0: passes of four)
};

static int store_option(gp_ctx *g, const OptDesc &o, int64_t value) {
    if (o.shape == OPT_RANGE && (value < o.lo || value > o.hi))
        return fail(GP_ERR_ARG, "%s out of range [%d, %d]", o.name, o.lo, o.hi);
    if (o.shape == OPT_FLOOR && value < o.lo) return fail(GP_ERR_ARG, "%s < %d", o.name, o.lo);
    if (o.shape == OPT_FLOOR) value = std::min<int64_t>(value, 1 << 20);
    if (o.shape == OPT_BOOL) value = value ? 1 : 0;
    g->*o.field = (int)value;
    return 0;
}

extern "C" int gp_set_option(gp_t *g, const char *name, int64_t value) {
    if (!g || !name) return fail(GP_ERR_ARG, "null argument");
    GP_DEAD_CHECK(g);
    for (const OptDesc &o : g_options) {
        if (strcmp(name, o.name)) continue;
        int rc = store_option(g, o, value);
        if (rc) return rc;
        // what a stored value invalidates
        if (o.field == &gp_ctx::lauum_panels) {
            // the factor stays, and with it invp_valid, lr_valid and predicted: only what the Ky^-1 route built is dropped
            g->wi_valid = false;
            g->li_valid = false;
            g->rows_calls_since_fit = 0;
            g->w_in_t2 = false;
        } else if (o.field == &gp_ctx::fmin_direct) {
            g->fmin_valid = false;
        } else if (o.field == &gp_ctx::emulate_fp64) {
            g->predicted = false;
        }
        return 0;
    }
    // the options that are not one int of the context
    if (!strcmp(name, "profile_min_tiles")) {
        if (value < 0) return fail(GP_ERR_ARG, "profile_min_tiles < 0");
        g->profile_min_tiles = value;
    } else if (!strcmp(name, "supertile")) {
        if (value < 0 || value > 64) return fail(GP_ERR_ARG, "supertile out of range");
        if (g->supertile != (int)value) {   // the cached tile orders belong to the old edge
            HIPCHK(hipSetDevice(g->device));
            HIPCHK(hipDeviceSynchronize());
            g->tile_lists.clear();
        }
        g->supertile = (int)value;
    } else if (!strcmp(name, "reserve_cus")) {
        if (value != g->bulk_reserved)
            return fail(GP_ERR_ARG, "reserve_cus is fixed when the device's streams are created (%d); set GPHIP_RESERVE_CUS "
                                    "before the first gp_create", g->bulk_reserved);
    } else if (!strcmp(name, "rns_interleave")) {
        rns_set_interleave((int)value);   // process-wide A/B switch of the residue GEMM's workgroup order (default 1)
    } else if (!strcmp(name, "debug_potrf_lds")) {
        if (value < 0 || value > (1 << 20)) return fail(GP_ERR_ARG, "debug_potrf_lds out of range");
        potrf_set_debug_lds((int)value);   // process-wide test hook: forces refused diagonal-tile launches (tests/test_gpu_round4.py)
    } else if (!strcmp(name, "debug_rows_skew")) {
        // test hook: shifts the arrival base of the one-location path's next pass, so that no workgroup finishes it
        g->pass.base[0] += (unsigned int)value;
    } else if (!strcmp(name, "small_m")) {
        if (value < 0 || value > 8) return fail(GP_ERR_ARG, "small_m out of range (0..8)");
        g->small_m = value;
        g->predicted = false;
    } else if (!strcmp(name, "mc_max")) {
        if (value < GP_TILE) return fail(GP_ERR_ARG, "mc_max < 128");
        g->mc_max = round_up(value, GP_TILE);
    } else
        return fail(GP_ERR_ARG, "unknown option %s", name);
    return 0;
}

// Test hook (tests/test_gpu_gemm_sched.py): one GEMM launch on host operands, through gemm() and so through the instance selection
// and the options every other launch of the context takes.
extern "C" int gp_debug_gemm(gp_t *g, int mode, double *C, const double *A, const double *B, int64_t ld, int K, int r0, int r1,
                             int c0, int c1, int tri) {
    if (!g || !C || !A || !B) return fail(GP_ERR_ARG, "null argument");
    GP_DEAD_CHECK(g);
    if (mode < 0 || mode > 1 || K < BK_MIN || K % BK_MIN || r0 < 0 || r1 <= r0 || c0 < 0 || c1 <= c0 || r1 > 256 || c1 > 256 ||
        (tri && r1 <= c1 - 1) || ld % 2 || ld < K || ld < (int64_t)c1 * GP_TILE)
        return fail(GP_ERR_ARG, "gp_debug_gemm: bad shape (mode %d K %d rows %d..%d columns %d..%d ld %ld)", mode, K, r0, r1, c0, c1, (long)ld);
    HIPCHK(hipSetDevice(g->device));
    const long ra = (long)r1 * GP_TILE, rb = (long)c1 * GP_TILE;
    DevBuf<double> dC, dA, dB;
    int rc;
    if ((rc = dC.reserve(ra * ld)) || (rc = dA.reserve(ra * ld)) || (rc = dB.reserve(rb * ld))) return rc;
    HIPCHK(hipMemcpyAsync(dC, C, (size_t)(ra * ld) * sizeof(double), hipMemcpyHostToDevice, g->s));
    HIPCHK(hipMemcpyAsync(dA, A, (size_t)(ra * ld) * sizeof(double), hipMemcpyHostToDevice, g->s));
    HIPCHK(hipMemcpyAsync(dB, B, (size_t)(rb * ld) * sizeof(double), hipMemcpyHostToDevice, g->s));
    gemm(g, g->s, mode, dC, ld, dA, ld, dB, ld, 1, K, TileSet{r0, r1, c0, c1, tri ? 1 : 0});
    HIPCHK(hipMemcpyAsync(C, dC, (size_t)(ra * ld) * sizeof(double), hipMemcpyDeviceToHost, g->s));
    GP_SYNC(g->s);
    return 0;
}

extern "C" int gp_synchronize(gp_t *g) {
    if (!g) return fail(GP_ERR_ARG, "null gp");
    GP_DEAD_CHECK(g);
    HIPCHK(hipSetDevice(g->device));
    GP_SYNC(g->s_panel);
    if (g->s_bulk) GP_SYNC(g->s_bulk);
    if (g->s_inv) GP_SYNC(g->s_inv);
    if (g->s_pred) GP_SYNC(g->s_pred);
    GP_SYNC(g->s);
    return 0;
}

extern "C" int gp_set_data(gp_t *g, const double *X, const double *Y, int64_t N, int D, int P) {
    if (!g || !X || !Y) return fail(GP_ERR_ARG, "null argument");
    GP_DEAD_CHECK(g);
    if (N < 1 || D < 1 || D > GP_MAX_D || P < 1 || P > GP_MAX_RHS)
        return fail(GP_ERR_ARG, "bad shape N=%ld D=%d P=%d (D <= %d, P <= %d)", (long)N, D, P, GP_MAX_D, GP_MAX_RHS);
    if (g->warp.n > 0 && P != 1)
        return fail(GP_ERR_STATE, "an output warp is on (gp_set_output_warp): it takes P = 1, switch it off before data with P = %d", P);
    HIPCHK(hipSetDevice(g->device));
    GP_SYNC(g->s);
    const long Npad = round_up(N, GP_TILE);
    if (Npad > g->capN || P > g->capP || !g->dA) {
        for (DevBuf<double> *b : {&g->dX, &g->dY, &g->dA, &g->dInvL, &g->dAlpha, &g->dW, &g->dMu}) b->release();
        const long capN = Npad;
        const int capP = std::max(P, g->capP);
        int rc;
        if ((rc = g->dX.reserve(capN * GP_MAX_D))) return rc;
        if ((rc = g->dY.reserve(capN * capP))) return rc;
        if ((rc = g->dA.reserve((capN + GP_MAX_RHS) * capN))) return rc;
        if ((rc = g->dInvL.reserve(capN * GP_TILE))) return rc;
        // the diagonal-tile kernel writes the lower block triangle of each inverted tile only (potrf.hip): the blocks above
        // it are zero from here on
        HIPCHK(hipMemsetAsync(g->dInvL, 0, sizeof(double) * capN * GP_TILE, g->s));
        if ((rc = g->dAlpha.reserve(capN * capP))) return rc;
        if ((rc = g->dW.reserve(capN * capP))) return rc;
        if ((rc = g->dMu.reserve(capN * 16))) return rc;
        g->capN = capN;
        g->capP = capP;
    }
    if (D != g->D) g->sp.Mz = g->sp.tM = g->sp.cR = 0;   // inducing inputs (and a sparse candidate table or point set) of another dimension are none of this data
    g->N = N;
    g->Npad = Npad;
    if (D != g->D) g->feas.K = 0;             // nor can a probability of feasibility cached over candidates of another width
    if (g->cost.Nc && g->cost.kp.D != D) {   // a surface of another width cannot serve these inputs
        g->cost.Nc = 0;
        g->cost_tab = 0;
    }
    if (g->mean.on() && (D != g->D || P != g->P)) g->mean.has_A = g->mean.has_b = g->mean.stale = false;   // A [D, P], b [P] of other data
    g->D = D;
    g->P = P;
    HIPCHK(hipMemcpyAsync(g->dX, X, sizeof(double) * N * D, hipMemcpyHostToDevice, g->s));
    HIPCHK(hipMemcpyAsync(g->dY, Y, sizeof(double) * N * P, hipMemcpyHostToDevice, g->s));
    if (g->mean.on()) {   // a resident mean function stays: the raw targets beside the residuals, rebuilt before the next factorisation
        int rc = g->dYraw.reserve(g->capN * (long)g->capP);
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(g->dYraw, Y, sizeof(double) * N * P, hipMemcpyHostToDevice, g->s));
        g->mean.stale = true;
    }
    if (g->warp.n > 0) {   // an active output warp is applied to the new targets
        int rc = warp_apply(g, true);
        if (rc) return rc;
    }
    GP_SYNC(g->s);
    g->have_data = true;
    fit_dropped(g);
    sparse_fit_dropped(g);
    g->ens.S = 0;   // the ensemble was fitted to the data that just left
    g->kp.D = D;
    return 0;
}

// The fork's Gower kernel option (GPy/GPy/kern/src/stationary.py:61-65,116-135; lengthscales = variable ranges,
// GPyOpt/GPyOpt/core/task/space.py:351-362).  Only K is Gower: Kdiag stays `variance` and the gradient
// formulas stay Euclidean in the fork.  Both are reproduced for the predictive gradients (gp_predict_grad, gp_acq_grad,
// gp_acq_lp_grad: Gower K(Xs, X) inside Euclidean gradients_X, see run_predict_grad) and for the hyper-parameter gradients
// (gp_lml_grad: Gower K in the variance gradient, Euclidean dK/dr in the lengthscale gradients, stationary.py:218-238).
static bool gower_refused(int kernel) { return kernel == GP_KERNEL_MATERN32 || kernel == GP_KERNEL_EXPONENTIAL; }

extern "C" int gp_set_gower(gp_t *g, int enable, const int *is_discrete, const double *range) {
    if (!g) return fail(GP_ERR_ARG, "null gp");
    GP_DEAD_CHECK(g);
    if (!g->have_data) return fail(GP_ERR_STATE, "gp_set_data first");
    if (enable && (!is_discrete || !range)) return fail(GP_ERR_ARG, "null argument");
    if (enable && g->have_params && gower_refused(g->kp.kernel))
        return fail(GP_ERR_ARG, "gp_set_gower: the Gower option covers GP_KERNEL_RBF and GP_KERNEL_MATERN52 only; gp_set_params chose kernel %d",
                    g->kp.kernel);
    g->kp.gower = enable ? 1 : 0;
    for (int d = 0; d < g->D && enable; ++d) {
        g->kp.gdisc[d] = is_discrete[d] ? 1 : 0;
        g->kp.gdiv[d] = is_discrete[d] ? 1.0 : range[d];
        if (!is_discrete[d] && !(range[d] > 0.0)) return fail(GP_ERR_ARG, "range of dimension %d must be positive", d);
    }
    fit_dropped(g);
    sparse_fit_dropped(g);
    return 0;
}

extern "C" int gp_set_params(gp_t *g, int kernel, int ard, double variance, const double *lengthscale, double noise) {
    if (!g || !lengthscale) return fail(GP_ERR_ARG, "null argument");
    GP_DEAD_CHECK(g);
    if (!g->have_data) return fail(GP_ERR_STATE, "gp_set_data must precede gp_set_params");
    if (kernel < GP_KERNEL_RBF || kernel > GP_KERNEL_EXPONENTIAL) return fail(GP_ERR_ARG, "unknown kernel %d", kernel);
    if (g->kp.gower && gower_refused(kernel))
        return fail(GP_ERR_ARG, "gp_set_params: kernel %d cannot follow gp_set_gower(enable): the Gower option covers GP_KERNEL_RBF and GP_KERNEL_MATERN52 only",
                    kernel);
    g->kp.kernel = kernel;
    g->kp.D = g->D;
    g->kp.variance = variance;
    for (int d = 0; d < g->D; ++d) g->kp.ls[d] = ard ? lengthscale[d] : lengthscale[0];
    g->ard = ard ? 1 : 0;
    laplace_dropped(g);   // (before the new noise is stored: dropping that state puts the old one back)
    g->noise = noise;
    g->have_params = true;
    fit_dropped(g);
    sparse_fit_dropped(g);
    return 0;
}

// ---- the same factorisation with one panel of look-ahead on three streams ----------------------------
// s_panel (high priority, every CU): the latency chain of panel J -- potrf tile, panel solve, in-panel
//          updates -- then the update of panel J+1's columns with panel J (so that chain J+1 can start);
// s_bulk  (masked off `reserve_cus` CUs, which therefore stay free for the chain's single-workgroup potrf
//          kernel whose 148 KB of LDS needs an otherwise empty CU): the update of every column right of
//          panel J+1 with panel J -- the dense contraction, >90 % of the flops;
// s       : everything before and after.
// Ordering: bulk(J) after chain(J); look-ahead update(J) after bulk(J-1) (both touch panel J+1's columns);
// bulk(J) after bulk(J-1) (stream order).  Column sets of concurrent kernels are disjoint by construction.
int ensure_bulk_stream(gp_ctx *g) {
    DevStreams d;
    int rc = get_streams(g->device, g->reserve_cus, &d);
    if (rc) return rc;
    g->s_bulk = d.bulk;
    g->bulk_reserved = d.reserved;
    return 0;
}

hipEvent_t la_event(gp_ctx *g, int kind, size_t i) {
    std::vector<hipEvent_t> &v = g->la_events[kind];
    while (v.size() <= i) {
        hipEvent_t e = nullptr;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
            // recorded, not swallowed: the entry point that ordered its streams through this event fails (la_events_ok)
            g->ev_error = true;
            e = nullptr;
        }
        v.push_back(e);
    }
    return v[i];
}
// Every stream-ordering event the last multi-stream section asked for exists (a failed hipEventCreateWithFlags would
// otherwise silently drop a dependency between two streams).
int la_events_ok(gp_ctx *g) {
    if (!g->ev_error) return 0;
    g->ev_error = false;
    for (auto &v : g->la_events) {   // drop the holes so that a later call retries the creation
        while (!v.empty() && v.back() == nullptr) v.pop_back();
        for (hipEvent_t e : v)
            if (!e) return fail(GP_ERR_HIP, "hipEventCreateWithFlags failed (stream-ordering event of the factorisation)");
    }
    return fail(GP_ERR_HIP, "hipEventCreateWithFlags failed (stream-ordering event of the factorisation)");
}

extern "C" int gp_get_alpha(gp_t *g, double *alpha) {
    if (!g || !alpha) return fail(GP_ERR_ARG, "null argument");
    GP_FITTED(g);
    std::vector<double> tmp((size_t)g->P * g->Npad);
    HIPCHK(hipMemcpy(tmp.data(), g->dAlpha, sizeof(double) * g->P * g->Npad, hipMemcpyDeviceToHost));
    for (long i = 0; i < g->N; ++i)
        for (int p = 0; p < g->P; ++p) alpha[i * g->P + p] = tmp[(size_t)p * g->Npad + i];
    return 0;
}

extern "C" int gp_get_chol(gp_t *g, double *L) {
    if (!g || !L) return fail(GP_ERR_ARG, "null argument");
    GP_FITTED(g);
    const long N = g->N;
    HIPCHK(hipMemcpy2D(L, sizeof(double) * N, g->dA, sizeof(double) * g->Npad, sizeof(double) * N, N,
                       hipMemcpyDeviceToHost));
    for (long i = 0; i < N; ++i)
        for (long j = i + 1; j < N; ++j) L[i * N + j] = 0.0;
    return 0;
}

extern "C" int gp_kernel_matrix(gp_t *g, double *K) {
    if (!g || !K) return fail(GP_ERR_ARG, "null argument");
    GP_DEAD_CHECK(g);
    if (!g->have_data || !g->have_params) return fail(GP_ERR_STATE, "set data and params first");
    HIPCHK(hipSetDevice(g->device));
    const long N = g->N;
    launch_kbuild(g->s, g->dA, g->Npad, g->dX, N, g->Npad, g->kp, 0.0, 1);
    GP_SYNC(g->s);
    HIPCHK(hipMemcpy2D(K, sizeof(double) * N, g->dA, sizeof(double) * g->Npad, sizeof(double) * N, N,
                       hipMemcpyDeviceToHost));
    factor_results_dropped(g);
    laplace_dropped(g);   // (a Laplace fit's factor went with dA as well: no state, gp_set_params' noise back)
    g->fitted = false;  // dA was overwritten; fmin_valid is left alone -- fmin was taken from dY and dAlpha, which still hold what they did
    return 0;
}

// kern.K(X, X2), stationary.py:107-140 with X2 given: the training inputs play the candidate role of cross_k_kernel
// (rows of the output), X2 the training role (columns), so K[N, M2] comes out row-major as the reference returns it.
extern "C" int gp_cross_kernel_matrix(gp_t *g, const double *X2, int64_t M2, double *K) {
    if (!g || !X2 || !K) return fail(GP_ERR_ARG, "null argument");
    GP_DEAD_CHECK(g);
    if (!g->have_data || !g->have_params) return fail(GP_ERR_STATE, "set data and params first");
    if (M2 < 1) return fail(GP_ERR_ARG, "M2 < 1");
    HIPCHK(hipSetDevice(g->device));
    const long N = g->N, Npad = g->Npad, M2pad = round_up(M2, GP_TILE);
    int rc;
    if ((rc = g->dX2.reserve((long)M2 * g->D))) return rc;
    if ((rc = g->dK2.reserve(Npad * M2pad))) return rc;
    HIPCHK(hipMemcpyAsync(g->dX2, X2, sizeof(double) * M2 * g->D, hipMemcpyHostToDevice, g->s));
    launch_cross_k(g->s, g->dK2, M2pad, g->dX, N, Npad, g->dX2, M2, M2pad, g->kp);
    GP_SYNC(g->s);
    HIPCHK(hipMemcpy2D(K, sizeof(double) * M2, g->dK2, sizeof(double) * M2pad, sizeof(double) * M2, N, hipMemcpyDeviceToHost));
    return 0;
}

/* ---- fit state (host scalars of the last fit, also what gp_comm_bcast_fit delivers to the receivers) ---- */
extern "C" int gp_get_fit_state(gp_t *g, double *lml, double *logdet, double *jitter) {
    if (!g) return fail(GP_ERR_ARG, "null gp");
    GP_DEAD_CHECK(g);
    if (!g->fitted) return fail(GP_ERR_STATE, "gp_fit first");
    if (lml) *lml = g->lml;
    if (logdet) *logdet = g->logdet;
    if (jitter) *jitter = g->jitter;
    return 0;
}
