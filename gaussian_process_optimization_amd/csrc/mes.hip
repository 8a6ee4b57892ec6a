// Max-value entropy search (Wang & Jegelka, ICML 2017; mirrored for a minimum): the rule over a table of rows, and the two
// reductions over a table's posterior that sampling the minimum's value y* needs --
//     log S(y) = sum_i log Phi((m_i - y) / s_i)      (the Gumbel approximation's survival function, independent marginals)
//     [min_i (m_i - nsig s_i), min_i (m_i + nsig s_i)]   (a bracket for its quantiles)
// -- so that no table-sized array travels to the host.  Plain wave64 code, one row per thread.
//
// Summation order of log S: ONE constant, MES_CHUNK = 256 rows per chunk.  A chunk is one workgroup: thread j holds row
// chunk * 256 + j (rows past M add 0), each of its four waves adds its 64 rows through the fixed xor tree (offsets 32, 16, .. 1),
// the four wave sums are added in wave order; the chunks' sums are added in chunk order by one thread per trial value.  A trial
// value's sum depends on that value and the table alone: not on G, not on its position, not on the call.  No atomics.
#include "acq_math.h"

// ---- the rule over a table ---------------------------------------------------------------------------------------------------------
__global__ void mes_acq_kernel(const double *ystar, int K, double y_mean, double y_std, const double *mean, const double *var,
                               const double *dmdx, const double *dvdx, long M, int D, double *out, double *dout) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    double f, c_m, c_s, ds_scale;
    mes_terms(ystar, K, y_mean, y_std, mean[i], var[i], f, c_m, c_s, ds_scale);
    out[i] = -f;
    if (!dout) return;
    for (int d = 0; d < D; ++d) {
        const double dm = dmdx[i * D + d] * y_std;
        const double ds = dvdx[i * D + d] * ds_scale;
        dout[i * D + d] = -(c_m * dm + c_s * ds);
    }
}
void launch_mes_acq(hipStream_t s, const double *ystar, int K, double y_mean, double y_std, const double *mean, const double *var,
                    const double *dmdx, const double *dvdx, long M, int D, double *out, double *dout) {
    if (M <= 0) return;
    GP_LAUNCH(mes_acq_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, ystar, K, y_mean, y_std, mean, var, dmdx, dvdx, M, D,
              out, dout);
}

// ---- the sampler's reductions ------------------------------------------------------------------------------------------------------
// (m, s) of a row as acq_terms un-normalises and clips them, every operation rounded on its own (no contraction: the bracket is
// NumPy's on the same posterior, bit for bit)
__device__ __forceinline__ void mes_row(double mean, double var, double y_mean, double y_std, double &m, double &s) {
#pragma clang fp contract(off)
    m = mean * y_std + y_mean;
    double v = var * (y_std * y_std);
    v = (v < 1e-10) ? 1e-10 : v;
    s = sqrt(v);
}
__device__ __forceinline__ double mes_wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(MES_CHUNK) void mes_logsurv_chunk_kernel(const double *mean, const double *var, long M, double y_mean,
                                                                      double y_std, MesY y, double *part) {
    __shared__ double sh[MES_CHUNK / 64][MES_MAX_G];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long i = (long)blockIdx.x * MES_CHUNK + tid;
    const bool live = i < M;
    double m = 0.0, s = 1.0;
    if (live) mes_row(mean[i], var[i], y_mean, y_std, m, s);   // loaded once, used for all G values
    for (int g = 0; g < y.G; ++g) {
        const double t = live ? gp_log_ndtr((m - y.y[g]) / s) : 0.0;
        const double w = mes_wave_sum(t);
        if (lane == 0) sh[wave][g] = w;
    }
    __syncthreads();
    if (tid < y.G) part[(long)blockIdx.x * MES_MAX_G + tid] = ((sh[0][tid] + sh[1][tid]) + sh[2][tid]) + sh[3][tid];
}
__global__ __launch_bounds__(MES_MAX_G) void mes_logsurv_final_kernel(const double *part, long nch, int G, double *res) {
    const int g = threadIdx.x;
    if (g >= G) return;
    double s = part[g];
    for (long c = 1; c < nch; ++c) s += part[c * MES_MAX_G + g];
    res[g] = s;
}
void launch_mes_logsurv(hipStream_t s, const double *mean, const double *var, long M, double y_mean, double y_std, const MesY &y,
                        double *part) {
    const long nch = mes_chunks(M);
    GP_LAUNCH(mes_logsurv_chunk_kernel, dim3((unsigned)nch), dim3(MES_CHUNK), 0, s, mean, var, M, y_mean, y_std, y, part);
    GP_LAUNCH(mes_logsurv_final_kernel, dim3(1), dim3(MES_MAX_G), 0, s, part, nch, y.G, part + nch * MES_MAX_G);
}

// min is exact and order-free: the chunks' minima, then the minimum of those (thread j of the second launch takes the chunks j,
// j + 256, ...)
__device__ __forceinline__ void mes_block_min2(double &a, double &b, double (*sh)[2]) {
    const int tid = threadIdx.x;
    for (int o = 32; o > 0; o >>= 1) {
        a = fmin(a, __shfl_xor(a, o));
        b = fmin(b, __shfl_xor(b, o));
    }
    if ((tid & 63) == 0) {
        sh[tid >> 6][0] = a;
        sh[tid >> 6][1] = b;
    }
    __syncthreads();
    a = fmin(fmin(sh[0][0], sh[1][0]), fmin(sh[2][0], sh[3][0]));
    b = fmin(fmin(sh[0][1], sh[1][1]), fmin(sh[2][1], sh[3][1]));
}
__global__ __launch_bounds__(MES_CHUNK) void mes_bracket_chunk_kernel(const double *mean, const double *var, long M, double y_mean,
                                                                      double y_std, double nsig, double *part) {
    __shared__ double sh[MES_CHUNK / 64][2];
    const long i = (long)blockIdx.x * MES_CHUNK + threadIdx.x;
    double a = INFINITY, b = INFINITY;
    if (i < M) {
#pragma clang fp contract(off)
        double m, s;
        mes_row(mean[i], var[i], y_mean, y_std, m, s);
        const double w = nsig * s;
        a = m - w;
        b = m + w;
    }
    mes_block_min2(a, b, sh);
    if (threadIdx.x == 0) {
        part[2 * (long)blockIdx.x] = a;
        part[2 * (long)blockIdx.x + 1] = b;
    }
}
__global__ __launch_bounds__(MES_CHUNK) void mes_bracket_final_kernel(const double *part, long nch, double *res) {
    __shared__ double sh[MES_CHUNK / 64][2];
    double a = INFINITY, b = INFINITY;
    for (long c = threadIdx.x; c < nch; c += MES_CHUNK) {
        a = fmin(a, part[2 * c]);
        b = fmin(b, part[2 * c + 1]);
    }
    mes_block_min2(a, b, sh);
    if (threadIdx.x == 0) {
        res[0] = a;
        res[1] = b;
    }
}
void launch_mes_bracket(hipStream_t s, const double *mean, const double *var, long M, double y_mean, double y_std, double nsig,
                        double *part) {
    const long nch = mes_chunks(M);
    GP_LAUNCH(mes_bracket_chunk_kernel, dim3((unsigned)nch), dim3(MES_CHUNK), 0, s, mean, var, M, y_mean, y_std, nsig, part);
    GP_LAUNCH(mes_bracket_final_kernel, dim3(1), dim3(MES_CHUNK), 0, s, part, nch, part + nch * MES_MAX_G);
}
