// fd_forecast.hip -- scores of a sample ensemble against the truth, per entry (NOT in the reference; the probabilistic protocol of
// the diffusion imputation / forecasting literature: CSDI, TimeGrad, TSDiff).  samples (n, K, T, C), truth (n, T, C); for every
// entry e = (series, t, c) with ensemble x_1 .. x_K and truth y:
//
//   crps[e]        = (1/K) sum_k |x_k - y| - (1/(2K^2)) sum_{j,k} |x_j - x_k|
//                  = (1/K) sum_k |x_k - y| - (1/K^2) sum_i (2i - K - 1) x_(i)         (x_(1) <= .. <= x_(K), i 1-based)
//   quantiles[q,e] = linear interpolation at position levels[q] (K - 1) of the sorted ensemble (numpy's "linear" method)
//   mean[e]        = (1/K) sum_k x_k
//
// A NaN truth or sample makes every output of its entry NaN and leaves the other entries alone.
//
// Layout: one workgroup of 256 threads owns a tile of E consecutive (t, c) entries of one series.  The K samples of an entry are
// strided by T C in memory, so the tile is staged as E columns of Kp = 2^ceil(log2 K) floats in LDS, [entry][k] with a row pitch
// of Kp + 1 (odd: the loads, E consecutive entries per sample row, and the sorting network, consecutive k of one column, are both
// free of bank conflicts); rows past K are +inf and sort to the end.  E Kp = 8192 (32 KiB of LDS, two workgroups per CU), E in
// [8, 256].  Each column is sorted in place by a bitonic network (log2 Kp (log2 Kp + 1) / 2 stages, one barrier each), then
// G = 256 / E lanes per entry accumulate the three sums in double and combine them by shuffles, and the entry's lanes share
// out the quantile levels.  The file is built without -fno-honor-nans (Makefile), so that its isnan tests are kept.
#include <algorithm>
#include <cmath>

#include "fd_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTileFloats = 8192;    // E * Kp
constexpr int kMaxK = 1024;

__global__ __launch_bounds__(kThreads) void k_ensemble_scores(const float* __restrict__ samples, const float* __restrict__ truth,
                                                              int n, int K, int TC, int lKp, int lE, int ntile,
                                                              const double* __restrict__ levels, int n_levels,
                                                              float* __restrict__ out_crps, float* __restrict__ out_q,
                                                              float* __restrict__ out_mean) {
    extern __shared__ float col[];               // E x (Kp + 1)
    __shared__ int bad[256];                     // per entry: a NaN sample was seen
    const int tid = threadIdx.x;
    const int Kp = 1 << lKp, E = 1 << lE;        // powers of two: the index arithmetic below is shifts and masks
    const int s = blockIdx.x / ntile, tc0 = (blockIdx.x % ntile) * E;
    const int pitch = Kp + 1;
    const size_t KTC = (size_t)K * TC;
    const float* xs = samples + (size_t)s * KTC;

    for (int j = tid; j < E; j += kThreads) bad[j] = 0;
    __syncthreads();
    // ---- stage: sample row k of the tile is E consecutive floats
    for (int idx = tid; idx < E * Kp; idx += kThreads) {
        const int j = idx & (E - 1), k = idx >> lE, tc = tc0 + j;
        float v = INFINITY;
        if (k < K && tc < TC) {
            v = xs[(size_t)k * TC + tc];
            if (isnan(v)) {
                bad[j] = 1;
                v = 0.f;                         // the entry's outputs become NaN; keep the network's comparisons ordered
            }
        }
        col[j * pitch + k] = v;
    }
    __syncthreads();
    // ---- sort every column ascending (bitonic: pair q of a stage compares i and i + stride, ascending where i & size == 0)
    const int half = Kp >> 1, lhalf = lKp - 1;
    for (int size = 2; size <= Kp; size <<= 1) {
        for (int ls = __builtin_ctz(size) - 1; ls >= 0; --ls) {
            const int stride = 1 << ls;
            for (int p = tid; p < E * half; p += kThreads) {
                const int j = p >> lhalf, q = p & (half - 1);
                const int i = ((q >> ls) << (ls + 1)) | (q & (stride - 1));
                float* c = col + j * pitch;
                const float a = c[i], b = c[i + stride];
                if ((a > b) == ((i & size) == 0)) {
                    c[i] = b;
                    c[i + stride] = a;
                }
            }
            __syncthreads();
        }
    }
    // ---- per entry: G lanes (aligned inside a wave) accumulate, then combine by shuffles
    const int G = kThreads / E;
    const int j = tid / G, g = tid % G, tc = tc0 + j;
    const bool live = tc < TC;
    const size_t e = (size_t)s * TC + tc;
    const float y = live ? truth[e] : 0.f;
    const float* c = col + j * pitch;
    double s_abs = 0.0, s_rank = 0.0, s_sum = 0.0;
    for (int k = g; k < K; k += G) {
        const double x = (double)c[k];
        s_abs += fabs(x - (double)y);
        s_rank += (double)(2 * k + 1 - K) * x;
        s_sum += x;
    }
    for (int m = 1; m < G; m <<= 1) {
        s_abs += __shfl_xor(s_abs, m, 64);
        s_rank += __shfl_xor(s_rank, m, 64);
        s_sum += __shfl_xor(s_sum, m, 64);
    }
    if (!live) return;
    const bool nan_entry = bad[j] != 0 || isnan(y);
    const float qnan = __builtin_nanf("");
    const double Kd = (double)K;
    if (g == 0) {
        if (out_crps) out_crps[e] = nan_entry ? qnan : (float)(s_abs / Kd - s_rank / (Kd * Kd));
        if (out_mean) out_mean[e] = nan_entry ? qnan : (float)(s_sum / Kd);
    }
    if (!out_q) return;
    const size_t plane = (size_t)n * TC;
    for (int qi = g; qi < n_levels; qi += G) {
        double pos = levels[qi] * (double)(K - 1);
        pos = fmin(fmax(pos, 0.0), (double)(K - 1));
        const int lo = (int)floor(pos);
        const int hi = lo + 1 < K ? lo + 1 : K - 1;
        const double t = pos - (double)lo, a = (double)c[lo], b = (double)c[hi], d = b - a;
        const double v = t < 0.5 ? a + d * t : b - d * (1.0 - t);      // numpy's _lerp
        out_q[(size_t)qi * plane + e] = nan_entry ? qnan : (float)v;
    }
}

}  // namespace

extern "C" int fd_ensemble_scores(fd_ctx* ctx, const float* samples, const float* truth, int n, int K, int T, int C,
                                  const double* levels, int n_levels, float* out_crps, float* out_quantiles, float* out_mean,
                                  void* stream) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, samples && truth, "fd_ensemble_scores: null pointer");
    FD_REQUIRE(ctx, n > 0 && T > 0 && C > 0, "fd_ensemble_scores: bad shape n=%d T=%d C=%d", n, T, C);
    FD_REQUIRE(ctx, K >= 1 && K <= kMaxK, "fd_ensemble_scores: K=%d outside [1, %d]", K, kMaxK);
    FD_REQUIRE(ctx, n_levels >= 0 && (n_levels == 0 || (levels && out_quantiles)),
               "fd_ensemble_scores: n_levels=%d needs levels and out_quantiles", n_levels);
    FD_REQUIRE(ctx, (long long)T * C < (1ll << 31), "fd_ensemble_scores: T*C too large");
    const int TC = T * C;
    int lKp = 0;
    while ((1 << lKp) < K) ++lKp;
    const int Kp = 1 << lKp;
    const int E = std::min(256, std::max(8, kTileFloats / Kp));
    const int lE = __builtin_ctz(E);
    const int ntile = (TC + E - 1) / E;
    FD_REQUIRE(ctx, (long long)n * ntile < (1ll << 31), "fd_ensemble_scores: n=%d too large for one launch", n);
    const size_t lds = sizeof(float) * (size_t)E * (Kp + 1);
    hipLaunchKernelGGL(k_ensemble_scores, dim3((unsigned)(n * ntile)), dim3(kThreads), lds, (hipStream_t)stream, samples, truth, n,
                       K, TC, lKp, lE, ntile, levels, n_levels, out_crps, n_levels ? out_quantiles : nullptr, out_mean);
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}
