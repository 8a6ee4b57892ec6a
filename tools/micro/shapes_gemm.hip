// Test tooling: throughput of the MFMA GEMM on the launch shapes the factorisation and the candidate solve use.
// build: hipcc --offload-arch=gfx950 -O3 -o shapes_gemm shapes_gemm.hip ../../gaussian_process_optimization_amd/csrc/gemm.o
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../gaussian_process_optimization_amd/csrc/gphip_internal.h"

// the library's launch-status slot (api_core.hip) is not linked into this stand-alone tool: report to stderr instead
void gp_note_hip(hipError_t e, const char *what, const char *file, int line) {
    if (e != hipSuccess) fprintf(stderr, "%s -> %s (%s:%d)\n", what, hipGetErrorString(e), file, line);
}
#define CHK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

// `shapes_gemm sched [runs]`: the 8-wave instance with the plain and with the scheduled K loop (GemmOpt::sched 0 / 1) on the same
// operands, alternating, `runs` timed runs of 10 launches each (default 5): the C3 candidate-update shape (79 x 98 tiles) and a
// trailing-update triangle of 100 row tiles, at K = 256, 768, 1536.  Before the timing each shape is computed once by either loop
// from the same C and the two results are compared bit for bit.
__global__ void count_diff_kernel(const unsigned long long *x, const unsigned long long *y, size_t n, unsigned long long *out) {
    unsigned long long c = 0;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) c += x[i] != y[i];
    if (c) atomicAdd(out, c);
}
static int sched_compare(int runs) {
    const long N = 16384, lda = N;
    double *A, *C, *T;
    unsigned long long *dcount, hcount = 0;
    CHK(hipMalloc(&A, (size_t)N * N * 8)); CHK(hipMalloc(&C, (size_t)N * N * 8)); CHK(hipMalloc(&T, (size_t)N * N * 8));
    CHK(hipMalloc(&dcount, 8));
    std::vector<double> hostA((size_t)N * 2048);
    for (size_t i = 0; i < hostA.size(); ++i) hostA[i] = (double)((i * 2654435761u) % 1000) / 1000.0 - 0.5;
    for (int r = 0; r < 8; ++r) CHK(hipMemcpy(A + (size_t)r * N * 2048, hostA.data(), hostA.size() * 8, hipMemcpyHostToDevice));
    hipEvent_t e0, e1; CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1));
    hipStream_t s; CHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    struct Shape { const char *name; TileSet ts; } shapes[2] = {{"rect 79x98 (C3 candidate update)", TileSet{0, 79, 0, 98, 0}},
                                                                {"tri 100 row tiles (trailing update)", TileSet{0, 100, 0, 100, 1}}};
    const int Ks[3] = {256, 768, 1536};
    const double *Aop = A + 8192, *Bop = A + (size_t)24 * 128 * lda + 4096;   // two different row panels of the random matrix
    printf("%-38s %5s  %-24s %-24s\n", "shape", "K", "plain TFLOP/s (runs)", "scheduled TFLOP/s (runs)");
    for (const Shape &sh : shapes)
        for (int K : Ks) {
            const long ntile = tileset_count(sh.ts);
            const double flop = 2.0 * 128 * 128 * K * ntile;
            GemmOpt o[2];
            for (int v = 0; v < 2; ++v) { o[v].stagger = 3; o[v].waves8 = 1; o[v].sched = v; }
            // bitwise: C and T start equal (the random matrix), one launch each
            CHK(hipMemcpyAsync(C, A, (size_t)N * N * 8, hipMemcpyDeviceToDevice, s));
            CHK(hipMemcpyAsync(T, A, (size_t)N * N * 8, hipMemcpyDeviceToDevice, s));
            launch_gemm_nt(s, 1, C, lda, Aop, lda, Bop, lda, 1, K, sh.ts, o[0]);
            launch_gemm_nt(s, 1, T, lda, Aop, lda, Bop, lda, 1, K, sh.ts, o[1]);
            CHK(hipMemsetAsync(dcount, 0, 8, s));
            count_diff_kernel<<<2048, 256, 0, s>>>((const unsigned long long *)C, (const unsigned long long *)T, (size_t)N * N, dcount);
            CHK(hipMemcpyAsync(&hcount, dcount, 8, hipMemcpyDeviceToHost, s));
            CHK(hipStreamSynchronize(s));
            if (hcount) { printf("%s K %d: %llu elements differ between the two loops\n", sh.name, K, hcount); return 1; }
            double tf[2][16];
            if (runs > 16) runs = 16;
            for (int r = 0; r < runs; ++r)
                for (int v = 0; v < 2; ++v) {
                    launch_gemm_nt(s, 1, C, lda, Aop, lda, Bop, lda, 1, K, sh.ts, o[v]);
                    CHK(hipEventRecord(e0, s));
                    for (int i = 0; i < 10; ++i) launch_gemm_nt(s, 1, C, lda, Aop, lda, Bop, lda, 1, K, sh.ts, o[v]);
                    CHK(hipEventRecord(e1, s)); CHK(hipEventSynchronize(e1));
                    float ms; CHK(hipEventElapsedTime(&ms, e0, e1));
                    tf[v][r] = flop / (ms / 10) / 1e9;
                }
            printf("%-38s %5d ", sh.name, K);
            for (int v = 0; v < 2; ++v) {
                printf(" ");
                for (int r = 0; r < runs; ++r) printf("%s%.2f", r ? "/" : "", tf[v][r]);
            }
            printf("\n");
            fflush(stdout);
        }
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "sched")) return sched_compare(argc > 2 ? atoi(argv[2]) : 5);
    const long N = 16384, lda = N;
    double *A, *C, *T;
    CHK(hipMalloc(&A, (size_t)(N + 128) * N * 8)); CHK(hipMalloc(&C, (size_t)(N + 128) * N * 8)); CHK(hipMalloc(&T, (size_t)(N + 128) * N * 8));
    CHK(hipMemset(C, 0, (size_t)N * N * 8)); CHK(hipMemset(T, 0, (size_t)N * N * 8));
    std::vector<double> hostA((size_t)N * 2048);
    for (size_t i = 0; i < hostA.size(); ++i) hostA[i] = (double)((i * 2654435761u) % 1000) / 1000.0 - 0.5;
    for (int r = 0; r < 8; ++r) CHK(hipMemcpy(A + (size_t)r * N * 2048, hostA.data(), hostA.size() * 8, hipMemcpyHostToDevice));
    hipEvent_t e0, e1; CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1));
    hipStream_t s0, s8;
    CHK(hipStreamCreateWithFlags(&s0, hipStreamNonBlocking));
    std::vector<uint32_t> mask(8, 0xffffffffu);
    for (int i = 0; i < 8; ++i) mask[0] &= ~(1u << i);
    CHK(hipExtStreamCreateWithCUMask(&s8, 8, mask.data()));
    auto run = [&](const char *name, hipStream_t s, double *Cc, const double *Aa, const double *Bb, int K, TileSet ts, GemmOpt o) -> int {
        long ntile = tileset_count(ts);
        launch_gemm_nt(s, 1, Cc, lda, Aa, lda, Bb, lda, 1, K, ts, o);
        CHK(hipStreamSynchronize(s));
        CHK(hipEventRecord(e0, s));
        for (int r = 0; r < 3; ++r) launch_gemm_nt(s, 1, Cc, lda, Aa, lda, Bb, lda, 1, K, ts, o);
        CHK(hipEventRecord(e1, s)); CHK(hipEventSynchronize(e1));
        float ms; CHK(hipEventElapsedTime(&ms, e0, e1)); ms /= 3;
        printf("%-44s tiles %6ld K %4d: %8.3f ms  %6.2f TFLOP/s\n", name, ntile, K, ms, 2.0 * 128 * 128 * K * ntile / ms / 1e9);
        fflush(stdout);
        return 0;
    };
    GemmOpt o; o.stagger = 3; o.waves8 = 1;
    GemmOpt o4; o4.stagger = 3; o4.waves8 = 0;
    char nm[128];
    for (int rep = 0; rep < 2; ++rep) {
        const int K = 768, c0 = 12;
        const long off = (long)(c0 - K / 128) * 128;
        if (run("tri  C=C A=B=Apanel (syrk)", s0, C, A + off, A + off, K, TileSet{0, 129, c0, 128, 1}, o)) return 1;
        if (run("tri  C=T A=Cpanel B=Apanel", s0, T, C + off, A + off, K, TileSet{0, 129, c0, 128, 1}, o)) return 1;
        if (run("tri  C=A itself (in-place syrk as in potrf)", s0, A, A + off, A + off, K, TileSet{0, 129, c0, 128, 1}, o)) return 1;
        if (run("rect 117x59 C=C A=B=Apanel", s0, C, A + off, A + off, K, TileSet{0, 117, 12, 71, 0}, o)) return 1;
        if (run("rect 117x59 C=T A=Cpanel B=Apanel", s0, T, C + off, A + off, K, TileSet{0, 117, 12, 71, 0}, o)) return 1;
        if (run("rect 59x117 C=C A=B=Apanel", s0, C, A + off, A + off, K, TileSet{0, 59, 12, 129, 0}, o)) return 1;
    }
    return 0;
}
