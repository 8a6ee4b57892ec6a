// hip_recorder: a stand-in for the HIP runtime (and RCCL) that runs NO kernel and needs no GPU.  Device memory is host memory
// from a bump allocator, copies are memcpy, and every call that orders or feeds a stream is written to $HIP_RECORDER_LOG in host
// order: launches (kernel, grid, block, LDS, stream; for gemm_nt_kernel every field of its GemmArgs, pointers as allocation index +
// offset; for the scoring kernels whose parameters are pointers and scalars only, every argument), hipEventRecord,
// hipStreamWaitEvent, memsets and copies (with destination and source), all-gathers, synchronisations, allocations.  Streams and
// events are numbered by first appearance.  The numbers an entry point returns are meaningless (zeros); the factorisation's status
// word reads 0, so a fit takes its first attempt ($HIP_RECORDER_FAIL=n: the first n status words read 1 instead, which walks the
// jitter ladder).  Two things are acted out because the host code waits for them: the finishing kernels of the fused rows passes
// (exact, sparse, ensemble) hand their ticket back ($HIP_RECORDER_NO_TICKET set to anything but 0, looked up at every launch: they
// withhold it, which walks the host's recovery), and the RCCL stand-ins give out communicators (of ONE rank: an all-gather copies
// send to receive).
// What it is for: a refactor of host code must leave this log unchanged.
//
// Build a recording libgphip.so from the objects of a normal build (make -C gaussian_process_optimization_amd/csrc), in a copy
// of the package outside the tree:
//   g++ -O1 -fPIC -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -c tools/hip_recorder.cpp -o hip_recorder.o
//   g++ -shared -fPIC gaussian_process_optimization_amd/csrc/*.o hip_recorder.o -o <copy>/gaussian_process_optimization_amd/libgphip.so
//   PYTHONPATH=<copy> HIP_RECORDER_LOG=case1.log python tools/stream_ops.py 1
// (struct GemmArgs below mirrors csrc/gemm.hip; ROWS_OUT_DOUBLES is the library's own, from its header.)
#pragma GCC diagnostic ignored "-Wattributes"   // (the header's ext_vector_type typedefs mean nothing to g++ and are not used here)
#include "../gaussian_process_optimization_amd/csrc/gphip_internal.h"
#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>
#include <cxxabi.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <sys/mman.h>
#include <vector>
// device memory: a bump allocator over one reserved range, so that a pointer prints as allocation index + offset
static char *g_base = nullptr;
static size_t g_top = 0;
static std::vector<std::pair<size_t, size_t>> g_allocs;   // offset, size
static void *dev_alloc(size_t n) {
    if (!g_base) g_base = (char *)mmap(nullptr, 1ul << 37, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    n = (n + 4095) / 4096 * 4096 + 4096;
    void *p = g_base + g_top;
    g_allocs.push_back({g_top, n});
    g_top += n;
    return p;
}
static std::string pname(const void *p) {
    char b[64];
    if (!p) return "null";
    const size_t o = (const char *)p - g_base;
    for (size_t i = g_allocs.size(); i-- > 0;)
        if (o >= g_allocs[i].first && o < g_allocs[i].first + g_allocs[i].second) { snprintf(b, 64, "a%zu+%zu", i, o - g_allocs[i].first); return b; }
    return "host";
}
struct GemmArgs { double *C; long ldc; const double *A; long lda; const double *B; long ldb; int b_mul, K, r0, r1, c0, c1, tri, k_tri, k_sub, k_end_tri, b_sub; long sC, sA, sB; const short *tile_list; int stagger, pair; };
static FILE *lg() { static FILE *f = fopen(getenv("HIP_RECORDER_LOG") ? getenv("HIP_RECORDER_LOG") : "/dev/null", "w"); return f; }
static std::map<const void *, std::string> &kn() { static std::map<const void *, std::string> m; return m; }
static std::map<const void *, int> g_s, g_e;
static int sid(const void *s) { auto it = g_s.find(s); if (it == g_s.end()) it = g_s.emplace(s, (int)g_s.size()).first; return it->second; }
static int eid(const void *e) { auto it = g_e.find(e); if (it == g_e.end()) it = g_e.emplace(e, (int)g_e.size()).first; return it->second; }
// every argument of a kernel whose parameters are pointers and scalars, by the parameter types in its mangled name (after the
// kernel's own name): P[K]<t> or a substitution S<n>_ is a pointer; d a double; i / j 32 bits; l / m / x / y 64 bits
static const char *const kScoring[] = {"argbest_kernel", "mask_kernel", "acq_kernel", "acq_grad_kernel", "lp_kernel", "lp_grad_kernel", "predict_reduce_kernel"};
static void log_args(FILE *f, const std::string &mangled, void **args) {
    for (const char *k : kScoring) {
        const std::string key = std::to_string(strlen(k)) + k;
        if (mangled.compare(0, 2 + key.size(), "_Z" + key)) continue;
        int n = 0;
        for (const char *t = mangled.c_str() + 2 + key.size(); *t; ++t, ++n) {
            if (*t == 'P') { t += (t[1] == 'K') ? 2 : 1; fprintf(f, " %s", pname(*(void **)args[n]).c_str()); }
            else if (*t == 'S') { while (*t != '_') ++t; fprintf(f, " %s", pname(*(void **)args[n]).c_str()); }
            else if (*t == 'd') fprintf(f, " %.17g", *(double *)args[n]);
            else if (*t == 'i' || *t == 'j') fprintf(f, " %d", *(int *)args[n]);
            else fprintf(f, " %lld", *(long long *)args[n]);
        }
        return;
    }
}
// The finishing kernels of the fused rows passes: in every one of them the pinned result block and the pass's ticket are the LAST
// TWO arguments, and the ticket goes behind the block.  (How many arguments a kernel has is read off its demangled signature.)
static const char *const kFinishing[] = {"rows_finish_kernel", "rows_mean_grad_kernel", "sparse_rows_kernel", "ens_finish_kernel"};
static void rows_ticket(const std::string &mangled, void **args) {
    bool finishing = false;
    for (const char *k : kFinishing) finishing = finishing || mangled.find(k) != std::string::npos;
    const char *off = getenv("HIP_RECORDER_NO_TICKET");
    if (!finishing || (off && atoi(off))) return;
    char *sig = abi::__cxa_demangle(mangled.c_str(), nullptr, nullptr, nullptr);
    if (!sig) return;
    const char *open = strrchr(sig, '(');
    int nargs = open && open[1] != ')' ? 1 : 0;
    for (const char *c = open; c && *c; ++c) nargs += *c == ',';
    free(sig);
    if (nargs >= 2) (*(double **)args[nargs - 2])[ROWS_OUT_DOUBLES] = *(double *)args[nargs - 1];
}
struct Cfg { dim3 g, b; size_t sh; hipStream_t s; };
static thread_local Cfg g_cfg;
extern "C" {
void **__hipRegisterFatBinary(const void *) { return (void **)malloc(8); }
void __hipUnregisterFatBinary(void **) {}
void __hipRegisterFunction(void **, const void *host, char *, const char *name, unsigned, void *, void *, void *, void *, int *) { kn()[host] = name; }
void __hipRegisterVar(void **, void *, char *, char *, int, size_t, int, int) {}
hipError_t __hipPushCallConfiguration(dim3 g, dim3 b, size_t sh, hipStream_t s) { g_cfg = Cfg{g, b, sh, s}; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3 *g, dim3 *b, size_t *sh, hipStream_t *s) { *g = g_cfg.g; *b = g_cfg.b; *sh = g_cfg.sh; *s = g_cfg.s; return hipSuccess; }
hipError_t hipLaunchKernel(const void *f, dim3 g, dim3 b, void **args, size_t sh, hipStream_t s) {
    const std::string name = kn().count(f) ? kn()[f] : "?";
    fprintf(lg(), "launch %s grid %u,%u,%u block %u,%u,%u shmem %zu s%d", name.c_str(), g.x, g.y, g.z, b.x, b.y, b.z, sh, sid(s));
    if (name.find("gemm_nt_kernel") != std::string::npos) {
        const GemmArgs &a = *(const GemmArgs *)args[0];
        fprintf(lg(), " C %s ldc %ld A %s lda %ld B %s ldb %ld b_mul %d K %d ts %d,%d,%d,%d,%d ktri %d ksub %d kend %d bsub %d s %ld,%ld,%ld list %s stag %d pair %d",
                pname(a.C).c_str(), a.ldc, pname(a.A).c_str(), a.lda, pname(a.B).c_str(), a.ldb, a.b_mul, a.K, a.r0, a.r1, a.c0, a.c1, a.tri, a.k_tri, a.k_sub,
                a.k_end_tri, a.b_sub, a.sC, a.sA, a.sB, pname(a.tile_list).c_str(), a.stagger, a.pair);
    }
    log_args(lg(), name, args);
    rows_ticket(name, args);
    fprintf(lg(), "\n");
    return hipSuccess;
}
hipError_t hipDeviceGetStreamPriorityRange(int *lo, int *hi) { *lo = 0; *hi = -1; return hipSuccess; }
hipError_t hipDeviceSynchronize() { fprintf(lg(), "devsync\n"); return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t *e) { *e = (hipEvent_t)malloc(1); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { *e = (hipEvent_t)malloc(1); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) { *ms = 0.f; return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { fprintf(lg(), "record e%d s%d\n", eid(e), sid(s)); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) { fprintf(lg(), "wait s%d e%d\n", sid(s), eid(e)); return hipSuccess; }
hipError_t hipExtStreamCreateWithCUMask(hipStream_t *s, uint32_t, const uint32_t *) { *s = (hipStream_t)malloc(1); return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { *s = (hipStream_t)malloc(1); return hipSuccess; }
hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned, int) { *s = (hipStream_t)malloc(1); return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t) { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t s) { fprintf(lg(), "sync s%d\n", sid(s)); return hipSuccess; }
hipError_t hipFree(void *p) { fprintf(lg(), "free %s\n", pname(p).c_str()); return hipSuccess; }
hipError_t hipHostFree(void *p) { free(p); return hipSuccess; }
hipError_t hipHostMalloc(void **p, size_t n, unsigned) { *p = calloc(1, n); return hipSuccess; }
hipError_t hipMalloc(void **p, size_t n) { *p = dev_alloc(n); fprintf(lg(), "malloc %zu\n", n); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipGetDeviceCount(int *n) { *n = 1; return hipSuccess; }
hipError_t hipGetDevicePropertiesR0600(hipDeviceProp_tR0600 *p, int) { memset(p, 0, sizeof *p); p->multiProcessorCount = 256; strcpy(p->name, "recorder"); strcpy(p->gcnArchName, "gfx950"); return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "recorder"; }
hipError_t hipGetLastError() { return hipSuccess; }
hipError_t hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind k) { fprintf(lg(), "memcpy %zu kind %d %s <- %s\n", n, (int)k, pname(d).c_str(), pname(s).c_str()); memcpy(d, s, n); return hipSuccess; }
hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind k, hipStream_t st) {
    static int fail = getenv("HIP_RECORDER_FAIL") ? atoi(getenv("HIP_RECORDER_FAIL")) : 0;
    fprintf(lg(), "memcpyAsync %zu kind %d s%d %s <- %s\n", n, (int)k, sid(st), pname(d).c_str(), pname(s).c_str());
    memcpy(d, s, n);
    if (n == sizeof(int) && k == hipMemcpyDeviceToHost && fail > 0 && fail--) *(int *)d = 1;   // a status word that reports a failed pivot
    return hipSuccess;
}
static void cp2d(void *d, size_t dp, const void *s, size_t sp, size_t w, size_t h) { for (size_t i = 0; i < h; ++i) memcpy((char *)d + i * dp, (const char *)s + i * sp, w); }
hipError_t hipMemcpy2D(void *d, size_t dp, const void *s, size_t sp, size_t w, size_t h, hipMemcpyKind k) { fprintf(lg(), "memcpy2D %zu x %zu kind %d %s <- %s\n", w, h, (int)k, pname(d).c_str(), pname(s).c_str()); cp2d(d, dp, s, sp, w, h); return hipSuccess; }
hipError_t hipMemcpy2DAsync(void *d, size_t dp, const void *s, size_t sp, size_t w, size_t h, hipMemcpyKind k, hipStream_t st) { fprintf(lg(), "memcpy2DAsync %zu x %zu kind %d s%d %s <- %s\n", w, h, (int)k, sid(st), pname(d).c_str(), pname(s).c_str()); cp2d(d, dp, s, sp, w, h); return hipSuccess; }
hipError_t hipMemcpyToSymbol(const void *, const void *, size_t, size_t, hipMemcpyKind) { return hipSuccess; }
hipError_t hipMemset(void *d, int v, size_t n) { fprintf(lg(), "memset %zu %s\n", n, pname(d).c_str()); if (n <= (1 << 20)) memset(d, v, n); return hipSuccess; }
hipError_t hipMemsetAsync(void *d, int v, size_t n, hipStream_t s) { fprintf(lg(), "memsetAsync %zu s%d %s\n", n, sid(s), pname(d).c_str()); if (n <= (1 << 20)) memset(d, v, n); return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
static ncclComm_t one_rank_comm() { return (ncclComm_t)malloc(1); }
ncclResult_t ncclAllGather(const void *send, void *recv, size_t count, ncclDataType_t, ncclComm_t, hipStream_t s) {
    fprintf(lg(), "allgather %zu s%d %s <- %s\n", count, sid(s), pname(recv).c_str(), pname(send).c_str());
    memmove(recv, send, count * sizeof(double));   // (ncclDouble is the only type the library gathers)
    return ncclSuccess;
}
ncclResult_t ncclBroadcast(const void *, void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) { return ncclSuccess; }
ncclResult_t ncclCommAbort(ncclComm_t) { return ncclSuccess; }
ncclResult_t ncclCommCount(const ncclComm_t, int *n) { *n = 1; return ncclSuccess; }
ncclResult_t ncclCommDestroy(ncclComm_t) { return ncclSuccess; }
ncclResult_t ncclCommInitAll(ncclComm_t *comms, int n, const int *) { for (int i = 0; i < n; ++i) comms[i] = one_rank_comm(); return ncclSuccess; }
ncclResult_t ncclCommInitRank(ncclComm_t *comm, int, ncclUniqueId, int) { *comm = one_rank_comm(); return ncclSuccess; }
ncclResult_t ncclCommUserRank(const ncclComm_t, int *r) { *r = 0; return ncclSuccess; }
const char *ncclGetErrorString(ncclResult_t) { return "recorder"; }
ncclResult_t ncclGetUniqueId(ncclUniqueId *id) { memset(id, 0, sizeof *id); return ncclSuccess; }
ncclResult_t ncclGetVersion(int *v) { *v = 0; return ncclSuccess; }
ncclResult_t ncclGroupEnd() { return ncclSuccess; }
ncclResult_t ncclGroupStart() { return ncclSuccess; }
}
