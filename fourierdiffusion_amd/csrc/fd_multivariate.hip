// fd_multivariate.hip -- multivariate scores of a sample ensemble against the truth, per series (NOT in the reference; Gneiting and
// Raftery 2007, Scheuerer and Hamill 2015, reported by the forecasting papers that follow CSDI and TimeGrad).  samples (n, K, T, C),
// truth (n, T, C), mask 1 = observed; H the hidden entries of a series (mask 0), d = |H|, x_1 .. x_K its members and y its truth:
//
//   energy     ES  = (1/K) sum_k ||x_k - y||_H - 1/(2 K^2) sum_{j,k} ||x_j - x_k||_H            (fair: 1/(2 K (K - 1)))
//   variogram  num = sum_{a<b in H, lag <= max_lag} w_ab (|y_a - y_b|^p - (1/K) sum_k |x_ka - x_kb|^p)^2,  den = sum w_ab
//              lag = |t_a - t_b| with t = e / C, w_ab = 1 or 1 / (1 + lag), p in {0.5, 1, 2}
//   ranks      below[e] = #{k : x_k < y}, equal[e] = #{k : x_k == y}, for every entry
//
// Both scores are P[i, j] = sum_r f(A[i, r] - A[j, r]) over row pairs i < j with a non-linear epilogue per pair, and share one
// tile kernel.  Energy: the rows are the K members plus the truth as row K (pairs (k, K) feed the first term, pairs (j, k) the
// second), the reduction runs over the T C entries, f = square, epilogue sqrt.  Variogram: the rows are the T C entries, the
// reduction runs over the K members, f = |.|^p, epilogue the weighted squared difference to the truth's |y_a - y_b|^p.
//
// Layout: a workgroup of 256 threads owns a 64 x 64 tile of row pairs of one series, a thread a 4 x 4 register tile.  Block
// (series, I, dj) owns row tiles I and J = I + dj: only the upper triangle exists, dj stops at the band |lag| <= max_lag allows, and
// a diagonal tile counts i < j only.  The reduction dimension is staged through LDS 64 at a time, 128 rows (64 of I, 64 of J):
//   energy     [row][r], pitch 68 floats: a member row is contiguous in memory, so lanes write consecutive r; a thread reads
//              4 consecutive r of its rows (ty + 16 a and tx + 16 b) as one 16-byte load, rows 68 floats apart land on
//              different 16-byte slots of the 256-byte bank row and lanes of one ty share an address
//   variogram  [k][row], pitch 128: a member's 64 consecutive entries are contiguous, so lanes write consecutive rows; a thread
//              reads its 4 consecutive rows (4 ty + a, 4 tx + b) of one member as one 16-byte load
// 34 KiB per workgroup, four workgroups per CU.  Differences are taken directly in fp32 (d = a - b; acc += d * d): the Gram
// expansion |a|^2 + |b|^2 - 2 a.b loses every digit on a tight ensemble far from the origin.  A staged chunk accumulates in fp32
// (at most 64 terms), chunks are carried in double, the epilogue runs in double.  Every tile writes one partial pair to the
// workspace; a second kernel adds a series' partials in fixed order.  No atomics: results are bit-reproducible and do not depend on
// n or on the series' position in the batch.
//
// Observed entries are skipped by select: the energy stage writes 0 for them, the variogram epilogue drops their pairs, so whatever
// they hold (NaN included) has no effect.  A NaN at a hidden entry makes the series' score NaN: in the energy score every hidden
// value meets the truth row, in the variogram score the always-present diagonal tile flags it.  The file is built without
// -fno-honor-nans (Makefile), so that its isnan tests are kept.
#include <cmath>

#include "fd_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 64;            // rows per side of a tile
constexpr int kChunk = 64;           // reduction items staged at a time
constexpr int kPitchE = 68;          // energy: [row][r], 4 (mod 64) floats
constexpr int kBufFloats = 2 * kTile * kPitchE;      // >= kChunk * 2 * kTile, the variogram's [k][row]
constexpr int kMaxK = 1024;
constexpr int kEnergy = 3;           // tile kernel mode; 0, 1, 2 are the variogram orders FD_VARIOGRAM_*

// sum of (v0, v1) over the workgroup in a fixed tree; every thread calls it, thread 0 holds the result
__device__ inline void block_sum2(double* red, int tid, double& v0, double& v1) {
    __syncthreads();
    red[tid] = v0;
    red[kThreads + tid] = v1;
    __syncthreads();
    for (int st = kThreads / 2; st > 0; st >>= 1) {
        if (tid < st) {
            red[tid] += red[tid + st];
            red[kThreads + tid] += red[kThreads + tid + st];
        }
        __syncthreads();
    }
    v0 = red[0];
    v1 = red[kThreads];
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void k_pair_tiles(const float* __restrict__ samples, const float* __restrict__ truth,
                                                         const uint8_t* __restrict__ mask, int mask_per_series, int K, int TC, int C,
                                                         int ntile, int W, int max_lag, int inverse_lag, double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float buf[kBufFloats];
    __shared__ float yv[2 * kTile];
    __shared__ int hidf[2 * kTile];
    __shared__ int side_cnt[2];
    __shared__ int bad;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int dj = blockIdx.x % (W + 1), rest = blockIdx.x / (W + 1);
    const int I = rest % ntile, s = rest / ntile, J = I + dj;
    double* out = part + 2 * (size_t)blockIdx.x;
    const float* xs = samples + (size_t)s * K * TC;
    const float* ys = truth + (size_t)s * TC;
    const uint8_t* ms = mask + (mask_per_series ? (size_t)s * TC : 0);
    if (J >= ntile) {                                       // below the triangle's edge: an empty partial
        if (tid == 0) out[0] = out[1] = 0.0;
        return;
    }
    float acc[4][4];
    double accd[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc[i][j] = 0.f;
            accd[i][j] = 0.0;
        }
    double v0 = 0.0, v1 = 0.0;

    if constexpr (MODE == kEnergy) {
        const int R = K + 1;                                // row K is the truth
        const int col = tid & 63, rw = tid >> 6;            // a wave stages one row of the chunk at a time
        for (int e0 = 0; e0 < TC; e0 += kChunk) {
            const int e = e0 + col;
            const bool hid = e < TC && ms[e] == 0;
            if (__ballot(hid) == 0) continue;               // every wave sees the same 64 entries: a uniform skip
            __syncthreads();
            for (int m = 0; m < 2 * kTile / 4; ++m) {
                const int r = rw + 4 * m;
                const int g = r < kTile ? I * kTile + r : J * kTile + r - kTile;
                float v = 0.f;                              // observed entries and rows past the truth: both sides 0, difference 0
                if (hid && g < R) v = g < K ? xs[(size_t)g * TC + e] : ys[e];
                buf[r * kPitchE + col] = v;
            }
            __syncthreads();
#pragma unroll 1
            for (int q = 0; q < kChunk / 4; ++q) {
                float4 a[4], b[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    a[i] = *reinterpret_cast<const float4*>(&buf[(ty + 16 * i) * kPitchE + 4 * q]);
                    b[i] = *reinterpret_cast<const float4*>(&buf[(kTile + tx + 16 * i) * kPitchE + 4 * q]);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float d = a[i].x - b[j].x;
                        acc[i][j] = fmaf(d, d, acc[i][j]);
                        d = a[i].y - b[j].y;
                        acc[i][j] = fmaf(d, d, acc[i][j]);
                        d = a[i].z - b[j].z;
                        acc[i][j] = fmaf(d, d, acc[i][j]);
                        d = a[i].w - b[j].w;
                        acc[i][j] = fmaf(d, d, acc[i][j]);
                    }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    accd[i][j] += (double)acc[i][j];
                    acc[i][j] = 0.f;
                }
        }
        // v0: sum of ||x_k - y|| over this tile's pairs (k, K); v1: sum of ||x_j - x_k|| over its pairs j < k
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int gi = I * kTile + ty + 16 * i, gj = J * kTile + tx + 16 * j;
                if (gi < gj && gj < R) {
                    const double nrm = sqrt(accd[i][j]);
                    if (gj == K) v0 += nrm;
                    else v1 += nrm;
                }
            }
        block_sum2(reinterpret_cast<double*>(buf), tid, v0, v1);
        if (tid == 0) {
            out[0] = v0;
            out[1] = v1;
        }
    } else {
        const int lastI = min(I * kTile + kTile - 1, TC - 1);
        if (max_lag >= 0 && (J * kTile) / C - lastI / C > max_lag) {        // the whole tile lies outside the band
            if (tid == 0) out[0] = out[1] = 0.0;
            return;
        }
        if (tid == 0) bad = 0;
        const int r = tid & 127, kk = tid >> 7;             // a wave stages 64 consecutive entries of one member
        const int g = r < kTile ? I * kTile + r : J * kTile + r - kTile;
        const bool hid = g < TC && ms[g] == 0;
        bool nan_seen = false;
        if (kk == 0) {
            const float y = hid ? ys[g] : 0.f;
            nan_seen = isnan(y);
            yv[r] = y;
            hidf[r] = hid ? 1 : 0;
            const unsigned long long live = __ballot(hid);
            if ((tid & 63) == 0) side_cnt[tid >> 6] = __popcll(live);
        }
        __syncthreads();
        if (side_cnt[0] == 0 || side_cnt[1] == 0) {         // no hidden row on one side: no pair
            if (tid == 0) out[0] = out[1] = 0.0;
            return;
        }
        for (int k0 = 0; k0 < K; k0 += kChunk) {
            const int kc = min(kChunk, K - k0);
            __syncthreads();
            for (int k = kk; k < kc; k += 2) {
                float v = 0.f;
                if (g < TC) v = xs[(size_t)(k0 + k) * TC + g];
                nan_seen |= hid && isnan(v);
                buf[k * (2 * kTile) + r] = v;
            }
            __syncthreads();
#pragma unroll 2
            for (int k = 0; k < kc; ++k) {
                const float4 a4 = *reinterpret_cast<const float4*>(&buf[k * (2 * kTile) + 4 * ty]);
                const float4 b4 = *reinterpret_cast<const float4*>(&buf[k * (2 * kTile) + kTile + 4 * tx]);
                const float a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float d = a[i] - b[j];
                        if constexpr (MODE == FD_VARIOGRAM_TWO) acc[i][j] = fmaf(d, d, acc[i][j]);
                        else if constexpr (MODE == FD_VARIOGRAM_ONE) acc[i][j] += fabsf(d);
                        else acc[i][j] += __builtin_amdgcn_sqrtf(fabsf(d));
                    }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    accd[i][j] += (double)acc[i][j];
                    acc[i][j] = 0.f;
                }
        }
        if (nan_seen) bad = 1;
        // v0: num, v1: den over this tile's pairs; an observed row's accumulators (whatever they hold) are never read
        const double invK = 1.0 / (double)K;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ri = 4 * ty + i, rj = kTile + 4 * tx + j;
                const int ei = I * kTile + ri, ej = J * kTile + rj - kTile;
                const int lag = ej / C - ei / C;
                if (hidf[ri] && hidf[rj] && ei < ej && (max_lag < 0 || lag <= max_lag)) {
                    const double dy = (double)yv[ri] - (double)yv[rj];
                    const double vy = MODE == FD_VARIOGRAM_TWO ? dy * dy : MODE == FD_VARIOGRAM_ONE ? fabs(dy) : sqrt(fabs(dy));
                    const double diff = vy - accd[i][j] * invK;
                    const double w = inverse_lag ? 1.0 / (1.0 + (double)lag) : 1.0;
                    v0 += w * diff * diff;
                    v1 += w;
                }
            }
        block_sum2(reinterpret_cast<double*>(buf), tid, v0, v1);            // its barriers also publish `bad`
        if (tid == 0) {
            out[0] = bad ? (double)__builtin_nanf("") : v0;
            out[1] = v1;
        }
    }
}

// one workgroup per series: its tiles' partials in ascending tile order (a fixed tree over fixed strides), its hidden count
__global__ __launch_bounds__(kThreads) void k_finish(const double* __restrict__ part, int tiles, int energy, int K, int fair, int TC,
                                                     const uint8_t* __restrict__ mask, int mask_per_series, double* __restrict__ out0,
                                                     double* __restrict__ out1, int32_t* __restrict__ out_hidden) {
    __shared__ double red[2 * kThreads];
    __shared__ int cnt[kThreads];
    const int tid = threadIdx.x, s = blockIdx.x;
    const double* p = part + 2 * (size_t)s * tiles;
    const uint8_t* ms = mask + (mask_per_series ? (size_t)s * TC : 0);
    double v0 = 0.0, v1 = 0.0;
    for (int i = tid; i < tiles; i += kThreads) {
        v0 += p[2 * i];
        v1 += p[2 * i + 1];
    }
    int c = 0;
    for (int e = tid; e < TC; e += kThreads) c += ms[e] == 0 ? 1 : 0;
    cnt[tid] = c;
    block_sum2(red, tid, v0, v1);
    for (int st = kThreads / 2; st > 0; st >>= 1) {
        if (tid < st) cnt[tid] += cnt[tid + st];
        __syncthreads();
    }
    if (tid != 0) return;
    const double qnan = (double)__builtin_nanf("");
    const double Kd = (double)K;
    if (out_hidden) out_hidden[s] = cnt[0];
    if (energy) {
        const double c2 = fair ? 1.0 / (Kd * (Kd - 1.0)) : 1.0 / (Kd * Kd);     // sum_{j,k} counts every pair j < k twice
        out0[s] = cnt[0] > 0 ? v0 / Kd - (K > 1 ? v1 * c2 : 0.0) : qnan;
    } else {
        out0[s] = v1 > 0.0 ? v0 : qnan;
        out1[s] = v1;
    }
}

__global__ __launch_bounds__(kThreads) void k_ranks(const float* __restrict__ samples, const float* __restrict__ truth, int K, int TC,
                                                    int32_t* __restrict__ below, int32_t* __restrict__ equal) {
    const int e = blockIdx.x * kThreads + threadIdx.x, s = blockIdx.y;
    if (e >= TC) return;
    const float* xs = samples + (size_t)s * K * TC + e;
    const float y = truth[(size_t)s * TC + e];
    int lo = 0, eq = 0;
    bool nan_seen = isnan(y);
    for (int k = 0; k < K; ++k) {
        const float x = xs[(size_t)k * TC];
        nan_seen |= isnan(x);
        lo += x < y ? 1 : 0;
        eq += x == y ? 1 : 0;
    }
    below[(size_t)s * TC + e] = nan_seen ? -1 : lo;
    equal[(size_t)s * TC + e] = nan_seen ? -1 : eq;
}

struct Plan {
    int TC, ntile, W;
    long long tiles;         // per series
};

// shared argument checks and the tile plan: ntile row tiles, dj in [0, W]; max_lag < 0: the whole upper triangle
int plan_for(fd_ctx* ctx, const char* who, int n, int K, int T, int C, bool energy, int max_lag, Plan* p) {
    FD_REQUIRE(ctx, n > 0 && T > 0 && C > 0, "%s: bad shape n=%d T=%d C=%d", who, n, T, C);
    FD_REQUIRE(ctx, K >= 1 && K <= kMaxK, "%s: K=%d outside [1, %d]", who, K, kMaxK);
    FD_REQUIRE(ctx, (long long)T * C < (1ll << 31) - kTile, "%s: T*C too large", who);
    p->TC = T * C;
    const int rows = energy ? K + 1 : p->TC;
    p->ntile = fd_cdiv(rows, kTile);
    long long W = p->ntile - 1;
    if (!energy && max_lag >= 0) {
        // rows 64 dj - 63 apart at the least are (64 dj - 63) / C - 1 time steps apart at the least
        const long long lag = max_lag < T - 1 ? max_lag : T - 1;
        const long long w = ((lag + 1) * C + kTile - 1) / kTile;
        if (w < W) W = w;
    }
    p->W = (int)W;
    p->tiles = (long long)p->ntile * (W + 1);
    FD_REQUIRE(ctx, (long long)n * p->tiles < (1ll << 31), "%s: n=%d too large for one launch (%lld tiles per series)", who, n,
               p->tiles);
    return FD_OK;
}

}  // namespace

extern "C" int fd_energy_score_workspace_bytes(fd_ctx* ctx, int n, int K, int T, int C, size_t* bytes) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, bytes, "fd_energy_score_workspace_bytes: null pointer");
    Plan p;
    if (int rc = plan_for(ctx, "fd_energy_score_workspace_bytes", n, K, T, C, true, -1, &p)) return rc;
    *bytes = 2 * sizeof(double) * (size_t)n * (size_t)p.tiles;
    return FD_OK;
}

extern "C" int fd_energy_score(fd_ctx* ctx, const float* samples, const float* truth, const uint8_t* mask_u8, int mask_per_series,
                               int n, int K, int T, int C, int fair, double* out_score, int32_t* out_hidden, void* work,
                               size_t work_bytes, void* stream) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, samples && truth && mask_u8 && out_score && out_hidden && work, "fd_energy_score: null pointer");
    Plan p;
    if (int rc = plan_for(ctx, "fd_energy_score", n, K, T, C, true, -1, &p)) return rc;
    FD_REQUIRE(ctx, !fair || K >= 2, "fd_energy_score: fair needs K >= 2, got K=%d", K);
    const size_t need = 2 * sizeof(double) * (size_t)n * (size_t)p.tiles;
    FD_REQUIRE(ctx, work_bytes >= need, "fd_energy_score: workspace of %zu bytes, needs %zu", work_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)work;
    hipLaunchKernelGGL(k_pair_tiles<kEnergy>, dim3((unsigned)(n * p.tiles)), dim3(kThreads), 0, st, samples, truth, mask_u8,
                       mask_per_series ? 1 : 0, K, p.TC, C, p.ntile, p.W, -1, 0, part);
    FD_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_finish, dim3((unsigned)n), dim3(kThreads), 0, st, part, (int)p.tiles, 1, K, fair ? 1 : 0, p.TC, mask_u8,
                       mask_per_series ? 1 : 0, out_score, (double*)nullptr, out_hidden);
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}

extern "C" int fd_variogram_score_workspace_bytes(fd_ctx* ctx, int n, int K, int T, int C, int max_lag, size_t* bytes) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, bytes, "fd_variogram_score_workspace_bytes: null pointer");
    Plan p;
    if (int rc = plan_for(ctx, "fd_variogram_score_workspace_bytes", n, K, T, C, false, max_lag, &p)) return rc;
    *bytes = 2 * sizeof(double) * (size_t)n * (size_t)p.tiles;
    return FD_OK;
}

extern "C" int fd_variogram_score(fd_ctx* ctx, const float* samples, const float* truth, const uint8_t* mask_u8,
                                  int mask_per_series, int n, int K, int T, int C, int order, int max_lag, int inverse_lag,
                                  double* out_num, double* out_den, int32_t* out_hidden, void* work, size_t work_bytes,
                                  void* stream) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, samples && truth && mask_u8 && out_num && out_den && work, "fd_variogram_score: null pointer");
    Plan p;
    if (int rc = plan_for(ctx, "fd_variogram_score", n, K, T, C, false, max_lag, &p)) return rc;
    FD_REQUIRE(ctx, order == FD_VARIOGRAM_HALF || order == FD_VARIOGRAM_ONE || order == FD_VARIOGRAM_TWO,
               "fd_variogram_score: order=%d is none of FD_VARIOGRAM_HALF, _ONE, _TWO", order);
    const size_t need = 2 * sizeof(double) * (size_t)n * (size_t)p.tiles;
    FD_REQUIRE(ctx, work_bytes >= need, "fd_variogram_score: workspace of %zu bytes, needs %zu", work_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)work;
    const dim3 grid((unsigned)(n * p.tiles)), block(kThreads);
    const int per = mask_per_series ? 1 : 0, lag = max_lag < 0 ? -1 : max_lag, inv = inverse_lag ? 1 : 0;
    if (order == FD_VARIOGRAM_HALF)
        hipLaunchKernelGGL(k_pair_tiles<FD_VARIOGRAM_HALF>, grid, block, 0, st, samples, truth, mask_u8, per, K, p.TC, C, p.ntile,
                           p.W, lag, inv, part);
    else if (order == FD_VARIOGRAM_ONE)
        hipLaunchKernelGGL(k_pair_tiles<FD_VARIOGRAM_ONE>, grid, block, 0, st, samples, truth, mask_u8, per, K, p.TC, C, p.ntile,
                           p.W, lag, inv, part);
    else
        hipLaunchKernelGGL(k_pair_tiles<FD_VARIOGRAM_TWO>, grid, block, 0, st, samples, truth, mask_u8, per, K, p.TC, C, p.ntile,
                           p.W, lag, inv, part);
    FD_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_finish, dim3((unsigned)n), block, 0, st, part, (int)p.tiles, 0, K, 0, p.TC, mask_u8, per, out_num, out_den,
                       out_hidden);
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}

extern "C" int fd_ensemble_ranks(fd_ctx* ctx, const float* samples, const float* truth, int n, int K, int T, int C, int32_t* below,
                                 int32_t* equal, void* stream) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, samples && truth && below && equal, "fd_ensemble_ranks: null pointer");
    FD_REQUIRE(ctx, n > 0 && T > 0 && C > 0, "fd_ensemble_ranks: bad shape n=%d T=%d C=%d", n, T, C);
    FD_REQUIRE(ctx, K >= 1 && K <= kMaxK, "fd_ensemble_ranks: K=%d outside [1, %d]", K, kMaxK);
    FD_REQUIRE(ctx, (long long)T * C < (1ll << 31) - kThreads, "fd_ensemble_ranks: T*C too large");
    FD_REQUIRE(ctx, n <= 65535, "fd_ensemble_ranks: n=%d too large for one launch (at most 65535 series)", n);
    const int TC = T * C;
    hipLaunchKernelGGL(k_ranks, dim3((unsigned)fd_cdiv(TC, kThreads), (unsigned)n), dim3(kThreads), 0, (hipStream_t)stream, samples,
                       truth, K, TC, below, equal);
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}
