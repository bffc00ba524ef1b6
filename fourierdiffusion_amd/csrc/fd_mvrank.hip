// fd_mvrank.hip -- multivariate rank histograms of a sample ensemble (NOT in the reference; Gneiting et al. 2008, Thorarinsdottir,
// Scheuerer and Heinz 2016, Smith and Hansen 2004 / Wilks 2004): the rank of the truth among the ensemble under a pre-rank that
// sees a whole series at once.  samples (n, K, T, C), truth (n, T, C), mask 1 = observed; for one series S = {x_0 = truth,
// x_1 .. x_K}, m = K + 1 points, H its hidden entries (mask 0).  For candidate j and entry e, over all m points i (j included):
// b = #{i : x_i[e] < x_j[e]}, a = #{i : x_i[e] > x_j[e]}, on the fp32 values as stored.
//
//   average     R_j = sum_{e in H} (m - a)                            the count of x_i[e] <= x_j[e]
//   band depth  B_j = sum_{e in H} [C(m,2) - C(b,2) - C(a,2)]          the pairs whose closed band holds x_j[e]
//   dominance   G_j = #{i : x_i[e] <= x_j[e] for every e in H}         (i = j counts)
//   mst         L_j = length of the Euclidean minimum spanning tree, over H, of S \ {x_j} (0 with fewer than two points left)
//
// and below = #{j >= 1 : rho_j < rho_0}, equal = #{j >= 1 : rho_j == rho_0}.  The three integer kinds accumulate in int64 and are
// written exactly as doubles (the entry points refuse C(m,2) T C >= 2^53).
//
// Kernels:
//   k_count<KIND>  average and band depth, by direct counting (no sort: ties need both b and a, which a count gives at once).  A
//                  workgroup owns one series and every S-th chunk of 8 consecutive entries; a chunk is staged for all m rows as
//                  [entry][row], pitch 1028 floats, so the 8 entries start in 8 different 16-byte slots of a bank row.  A work item
//                  is (candidate j, entry e), e fastest over the lanes: it walks the m rows of its entry four at a time
//                  (ds_read_b128, eight addresses per wave-instruction, each shared by the lanes of one e), the 8 entries of a
//                  candidate are added by three lane exchanges and go to the candidate's int64 accumulator in the LDS, which one
//                  thread owns.  One partial per (series, split) goes to the workspace.
//   k_tiles<DOM>   64 x 64 tiles of point pairs (i, j) of one series, a thread a 4 x 4 register tile, the entries staged 64 at a
//                  time as [row][e], pitch 68 (the layout of fd_multivariate.hip's energy tiles).  Dominance: one violation flag
//                  per pair, "x_i[e] > x_j[e] at some hidden e"; the tile's count of unviolated i per j is one partial.  Distances
//                  (mst): (double)a - (double)b, squared and summed in double in ascending entry order, sqrt, into the m x m
//                  matrix of the series in the workspace.  Both directions of a pair are computed (the full square of tiles): the
//                  matrix is symmetric bit for bit, and the fp64 work is m^2 d fused multiply-adds per series.
//   k_prim         one (series, left-out j) per workgroup: Prim's algorithm on the distance matrix, keys in the LDS (a thread owns
//                  the vertices tid, tid + threads, ..), the argmin a fixed tree (xor exchanges inside a wave, then the waves in
//                  ascending order) that breaks ties to the lower index; the length is summed in selection order.
//   k_rank_finish  one workgroup per series: adds the partials in ascending order, writes prerank, below, equal and hidden.
//
// Observed entries are skipped by select (staged as 0 on every row, or not visited).  A NaN at a hidden entry, in the truth or in a
// member, poisons its series and no other: every staging pass flags it, the finishing kernel writes below = equal = -1 and the
// pre-ranks -1 (NaN for mst).  A series without a hidden entry gets equal pre-ranks: below 0, equal K, hidden 0.  No atomics; the
// integer sums are exact and the distance sums run in a fixed order, so a series' outputs do not depend on n, on its position or on
// the split, and two runs are bit-identical.  Built without -fno-honor-nans (Makefile): the isnan tests are kept.
#include <climits>
#include <cmath>

#include "fd_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxM = 1024;                      // points per series, truth included
constexpr int kE = 8;                            // k_count: entries per staged chunk
constexpr int kPitchC = kMaxM + 4;               // k_count: [entry][row]; 4 (mod 64) floats
constexpr int kTile = 64;                        // k_tiles: rows per side
constexpr int kChunk = 64;                       // k_tiles: entries staged at a time
constexpr int kPitchT = 68;                      // k_tiles: [row][e], 4 (mod 64) floats
constexpr int kTargetBlocks = 2048;              // k_count: split a series' chunks until the grid has about this many workgroups

__device__ inline float point_value(const float* xs, const float* ys, int row, size_t TC, int e) {
    return row == 0 ? ys[e] : xs[(size_t)(row - 1) * TC + e];
}

template <int KIND>
__global__ __launch_bounds__(kThreads) void k_count(const float* __restrict__ samples, const float* __restrict__ truth,
                                                    const uint8_t* __restrict__ mask, int mask_per_series, int K, int TC, int S,
                                                    long long* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float buf[kE * kPitchC];
    __shared__ long long acc[kMaxM];
    const int tid = threadIdx.x, p = blockIdx.x % S, s = blockIdx.x / S, m = K + 1;
    const float* xs = samples + (size_t)s * K * TC;
    const float* ys = truth + (size_t)s * TC;
    const uint8_t* ms = mask + (mask_per_series ? (size_t)s * TC : 0);
    const int m4 = (m + 3) & ~3, nchunk = (TC + kE - 1) / kE, items = m * kE;
    const int cm2 = m * (m - 1) / 2;
    for (int j = tid; j < m; j += kThreads) acc[j] = 0;
    bool nan_seen = false;
    for (int c = p; c < nchunk; c += S) {
        const int e0 = c * kE;
        unsigned hm = 0;                                    // the chunk's hidden entries: the same in every thread
#pragma unroll
        for (int i = 0; i < kE; ++i) hm |= (e0 + i < TC && ms[e0 + i] == 0) ? 1u << i : 0u;
        if (hm == 0) continue;
        __syncthreads();
        for (int w = tid; w < m4 * kE; w += kThreads) {
            const int e = w & (kE - 1), r = w >> 3;
            float v = __builtin_nanf("");                   // rows past m: NaN is neither below nor above anything
            if (r < m) {
                v = 0.f;
                if ((hm >> e) & 1u) {
                    v = point_value(xs, ys, r, (size_t)TC, e0 + e);
                    nan_seen |= isnan(v);
                }
            }
            buf[e * kPitchC + r] = v;
        }
        __syncthreads();
        for (int w = tid; w < items; w += kThreads) {
            const int e = w & (kE - 1), j = w >> 3;
            int term = 0;
            if ((hm >> e) & 1u) {
                const float* col = buf + e * kPitchC;
                const float xj = col[j];
                int b = 0, a = 0;
                for (int i = 0; i < m4; i += 4) {
                    const float4 v = *reinterpret_cast<const float4*>(col + i);
                    a += (v.x > xj ? 1 : 0) + (v.y > xj ? 1 : 0) + (v.z > xj ? 1 : 0) + (v.w > xj ? 1 : 0);
                    if constexpr (KIND == FD_PRERANK_BAND_DEPTH)
                        b += (v.x < xj ? 1 : 0) + (v.y < xj ? 1 : 0) + (v.z < xj ? 1 : 0) + (v.w < xj ? 1 : 0);
                }
                if constexpr (KIND == FD_PRERANK_BAND_DEPTH) term = cm2 - b * (b - 1) / 2 - a * (a - 1) / 2;
                else term = m - a;
            }
            // the 8 entries of candidate j sit in 8 neighbouring lanes, all of them inside this loop: at most 8 C(m,2) < 2^23
            term += __shfl_xor(term, 1);
            term += __shfl_xor(term, 2);
            term += __shfl_xor(term, 4);
            if (e == 0) acc[j] += term;                     // acc[j] belongs to this thread in every chunk
        }
    }
    const int bad = __syncthreads_or(nan_seen ? 1 : 0);
    long long* out = part + (size_t)blockIdx.x * (m + 1);
    for (int j = tid; j < m; j += kThreads) out[j] = acc[j];
    if (tid == 0) out[m] = bad;
}

// DOM: part (n, ntile, m + ntile) int64, slab I holds the counts of tile row I and its flags; else dist (n, m, m) and flags
// (n, ntile, ntile) int32
template <bool DOM>
__global__ __launch_bounds__(kThreads) void k_tiles(const float* __restrict__ samples, const float* __restrict__ truth,
                                                    const uint8_t* __restrict__ mask, int mask_per_series, int K, int TC, int ntile,
                                                    long long* __restrict__ part, double* __restrict__ dist,
                                                    int32_t* __restrict__ flags) {
    __shared__ __attribute__((aligned(16))) float buf[2 * kTile * kPitchT];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, m = K + 1;
    const int J = blockIdx.x % ntile, rest = blockIdx.x / ntile, I = rest % ntile, s = rest / ntile;
    const float* xs = samples + (size_t)s * K * TC;
    const float* ys = truth + (size_t)s * TC;
    const uint8_t* ms = mask + (mask_per_series ? (size_t)s * TC : 0);
    int viol[4][4];
    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            viol[i][j] = 0;
            acc[i][j] = 0.0;
        }
    bool nan_seen = false;
    const int col = tid & 63, rw = tid >> 6;                // a wave stages one row of the chunk at a time
    for (int e0 = 0; e0 < TC; e0 += kChunk) {
        const int e = e0 + col;
        const bool hid = e < TC && ms[e] == 0;
        if (__ballot(hid) == 0) continue;                   // every wave sees the same 64 entries: a uniform skip
        __syncthreads();
        for (int q = 0; q < 2 * kTile / 4; ++q) {
            const int r = rw + 4 * q;
            const int g = r < kTile ? I * kTile + r : J * kTile + r - kTile;
            float v = 0.f;                                  // observed entries and rows past m: 0 on both sides
            if (hid && g < m) {
                v = point_value(xs, ys, g, (size_t)TC, e);
                nan_seen |= isnan(v);
            }
            buf[r * kPitchT + col] = v;
        }
        __syncthreads();
#pragma unroll 1
        for (int q = 0; q < kChunk / 4; ++q) {
            float4 a4[4], b4[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                a4[i] = *reinterpret_cast<const float4*>(&buf[(ty + 16 * i) * kPitchT + 4 * q]);
                b4[i] = *reinterpret_cast<const float4*>(&buf[(kTile + tx + 16 * i) * kPitchT + 4 * q]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if constexpr (DOM) {
                        // counted, not or-ed: a compare and an add with carry per term, all in vector registers (at most T*C)
                        viol[i][j] += a4[i].x > b4[j].x ? 1 : 0;
                        viol[i][j] += a4[i].y > b4[j].y ? 1 : 0;
                        viol[i][j] += a4[i].z > b4[j].z ? 1 : 0;
                        viol[i][j] += a4[i].w > b4[j].w ? 1 : 0;
                    } else {
                        double d = (double)a4[i].x - (double)b4[j].x;
                        acc[i][j] = fma(d, d, acc[i][j]);
                        d = (double)a4[i].y - (double)b4[j].y;
                        acc[i][j] = fma(d, d, acc[i][j]);
                        d = (double)a4[i].z - (double)b4[j].z;
                        acc[i][j] = fma(d, d, acc[i][j]);
                        d = (double)a4[i].w - (double)b4[j].w;
                        acc[i][j] = fma(d, d, acc[i][j]);
                    }
                }
        }
    }
    const int bad = __syncthreads_or(nan_seen ? 1 : 0);     // its barrier also ends the last chunk's reads of buf
    if constexpr (DOM) {
        int* cnt = reinterpret_cast<int*>(buf);             // [ty][column of the tile]
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int c = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) c += (I * kTile + ty + 16 * i < m && viol[i][j] == 0) ? 1 : 0;
            cnt[ty * kTile + tx + 16 * j] = c;
        }
        __syncthreads();
        long long* out = part + ((size_t)s * ntile + I) * (size_t)(m + ntile);
        if (tid < kTile) {
            int c = 0;
            for (int r = 0; r < 16; ++r) c += cnt[r * kTile + tid];
            const int gj = J * kTile + tid;
            if (gj < m) out[gj] = c;
        }
        if (tid == 0) out[m + J] = bad;
    } else {
        double* ds = dist + (size_t)s * m * m;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int gi = I * kTile + ty + 16 * i, gj = J * kTile + tx + 16 * j;
                if (gi < m && gj < m) ds[(size_t)gi * m + gj] = sqrt(acc[i][j]);
            }
        if (tid == 0) flags[((size_t)s * ntile + I) * ntile + J] = bad;
    }
}

// Prim's algorithm on the points of series s without point j; blockDim.x is 64, 128 or 256
__global__ __launch_bounds__(kThreads) void k_prim(const double* __restrict__ dist, int m, double* __restrict__ prerank) {
    __shared__ double key[kMaxM];                           // distance to the tree; -1: in the tree or left out
    __shared__ double wkey[2][kThreads / 64];
    __shared__ int widx[2][kThreads / 64];
    const int tid = threadIdx.x, nt = blockDim.x, nwave = nt >> 6;
    const int j = blockIdx.x % m, s = blockIdx.x / m;
    const double* ds = dist + (size_t)s * m * m;
    const int root = j == 0 ? 1 : 0;
    double total = 0.0;
    if (m >= 3) {
        for (int v = tid; v < m; v += nt) key[v] = (v == j || v == root) ? -1.0 : ds[(size_t)root * m + v];
        int par = 0;
        for (int step = 0; step < m - 2; ++step) {
            double bk = INFINITY;
            int bi = INT_MAX;
            for (int v = tid; v < m; v += nt) {             // ascending v: a tie keeps the lower index; a NaN key is never taken
                const double k = key[v];
                if (k >= 0.0 && k < bk) {
                    bk = k;
                    bi = v;
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const double ok = __shfl_xor(bk, off);
                const int oi = __shfl_xor(bi, off);
                if (ok < bk || (ok == bk && oi < bi)) {
                    bk = ok;
                    bi = oi;
                }
            }
            if ((tid & 63) == 0) {
                wkey[par][tid >> 6] = bk;
                widx[par][tid >> 6] = bi;
            }
            __syncthreads();
            bk = wkey[par][0];
            bi = widx[par][0];
            for (int w = 1; w < nwave; ++w) {
                const double ok = wkey[par][w];
                const int oi = widx[par][w];
                if (ok < bk || (ok == bk && oi < bi)) {
                    bk = ok;
                    bi = oi;
                }
            }
            par ^= 1;
            if (bi == INT_MAX) break;                       // NaN distances (a poisoned series): the same in every thread
            total += bk;
            const double* row = ds + (size_t)bi * m;
            for (int v = tid; v < m; v += nt) {
                const double k = key[v];
                if (v == bi) key[v] = -1.0;
                else if (k >= 0.0) {
                    const double d = row[v];
                    if (d < k) key[v] = d;
                }
            }
        }
    }
    if (tid == 0) prerank[(size_t)s * m + j] = total;
}

// mst: the pre-ranks are in prerank already, flags int32 (nflag per series).  Else part int64 (P slabs of m + nflag per series,
// the flags behind the m counts of a slab).
__global__ __launch_bounds__(kThreads) void k_rank_finish(int mst, const long long* __restrict__ part, int P, int nflag,
                                                          const int32_t* __restrict__ flags, int m, int TC,
                                                          const uint8_t* __restrict__ mask, int mask_per_series,
                                                          double* __restrict__ prerank, int32_t* __restrict__ below,
                                                          int32_t* __restrict__ equal, int32_t* __restrict__ hidden) {
    __shared__ double rho[kMaxM];
    __shared__ int red[3][kThreads];
    const int tid = threadIdx.x, s = blockIdx.x;
    const uint8_t* ms = mask + (mask_per_series ? (size_t)s * TC : 0);
    double* pr = prerank + (size_t)s * m;
    const size_t W = (size_t)m + nflag;
    const long long* ps = part + (size_t)s * P * W;
    int bad = 0;
    if (mst) {
        for (int i = tid; i < nflag; i += kThreads) bad |= flags[(size_t)s * nflag + i];
        for (int j = tid; j < m; j += kThreads) rho[j] = pr[j];
    } else {
        for (int i = tid; i < P * nflag; i += kThreads) bad |= ps[(size_t)(i / nflag) * W + m + i % nflag] != 0 ? 1 : 0;
        for (int j = tid; j < m; j += kThreads) {
            long long v = 0;
            for (int p = 0; p < P; ++p) v += ps[(size_t)p * W + j];
            rho[j] = (double)v;                             // exact: below 2^53
        }
    }
    bad = __syncthreads_or(bad);
    const double r0 = rho[0];
    int lo = 0, eq = 0, hid = 0;
    for (int j = 1 + tid; j < m; j += kThreads) {
        lo += rho[j] < r0 ? 1 : 0;
        eq += rho[j] == r0 ? 1 : 0;
    }
    for (int e = tid; e < TC; e += kThreads) hid += ms[e] == 0 ? 1 : 0;
    red[0][tid] = lo;
    red[1][tid] = eq;
    red[2][tid] = hid;
    __syncthreads();
    for (int st = kThreads / 2; st > 0; st >>= 1) {
        if (tid < st) {
            red[0][tid] += red[0][tid + st];
            red[1][tid] += red[1][tid + st];
            red[2][tid] += red[2][tid + st];
        }
        __syncthreads();
    }
    const double poisoned = mst ? (double)__builtin_nanf("") : -1.0;
    for (int j = tid; j < m; j += kThreads) pr[j] = bad ? poisoned : rho[j];
    if (tid == 0) {
        below[s] = bad ? -1 : red[0][0];
        equal[s] = bad ? -1 : red[1][0];
        if (hidden) hidden[s] = red[2][0];
    }
}

struct Plan {
    int TC, m, ntile, S;      // S: the splits of a series' entry chunks (average, band depth)
    size_t bytes, flag_offset;
};

int plan_for(fd_ctx* ctx, const char* who, int kind, int n, int K, int T, int C, Plan* p) {
    FD_REQUIRE(ctx, kind == FD_PRERANK_AVERAGE || kind == FD_PRERANK_BAND_DEPTH || kind == FD_PRERANK_DOMINANCE ||
                        kind == FD_PRERANK_MST,
               "%s: kind=%d is none of FD_PRERANK_AVERAGE, _BAND_DEPTH, _DOMINANCE, _MST", who, kind);
    FD_REQUIRE(ctx, n > 0 && T > 0 && C > 0, "%s: bad shape n=%d T=%d C=%d", who, n, T, C);
    FD_REQUIRE(ctx, K >= 1 && K <= kMaxM - 1, "%s: K=%d outside [1, %d]", who, K, kMaxM - 1);
    FD_REQUIRE(ctx, (long long)T * C < (1ll << 31) - kTile, "%s: T*C too large", who);
    const long long m = K + 1, TC = (long long)T * C;
    FD_REQUIRE(ctx, m * (m - 1) / 2 * TC < (1ll << 53), "%s: T*C too large: C(K+1, 2) * T*C = %lld is not below 2^53", who,
               m * (m - 1) / 2 * TC);
    p->TC = (int)TC;
    p->m = (int)m;
    p->ntile = fd_cdiv(m, kTile);
    const long long nchunk = (TC + kE - 1) / kE;
    long long S = (kTargetBlocks + n - 1) / n;
    if (S > nchunk) S = nchunk;
    p->S = (int)S;
    long long blocks, bytes;
    p->flag_offset = 0;
    if (kind == FD_PRERANK_MST) {
        blocks = (long long)n * (p->ntile * p->ntile > m ? p->ntile * p->ntile : m);
        p->flag_offset = sizeof(double) * (size_t)n * (size_t)m * (size_t)m;
        bytes = (long long)p->flag_offset + (long long)sizeof(int32_t) * n * p->ntile * p->ntile;
    } else if (kind == FD_PRERANK_DOMINANCE) {
        blocks = (long long)n * p->ntile * p->ntile;
        bytes = (long long)sizeof(long long) * n * p->ntile * (m + p->ntile);
    } else {
        blocks = (long long)n * S;
        bytes = (long long)sizeof(long long) * n * S * (m + 1);
    }
    FD_REQUIRE(ctx, blocks < (1ll << 31), "%s: n=%d too large for one launch (%lld workgroups)", who, n, blocks);
    p->bytes = (size_t)bytes;
    return FD_OK;
}

}  // namespace

extern "C" int fd_multivariate_ranks_workspace_bytes(fd_ctx* ctx, int kind, int n, int K, int T, int C, size_t* bytes) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, bytes, "fd_multivariate_ranks_workspace_bytes: null pointer");
    Plan p;
    if (int rc = plan_for(ctx, "fd_multivariate_ranks_workspace_bytes", kind, n, K, T, C, &p)) return rc;
    *bytes = p.bytes;
    return FD_OK;
}

extern "C" int fd_multivariate_ranks(fd_ctx* ctx, int kind, const float* samples, const float* truth, const uint8_t* mask_u8,
                                     int mask_per_series, int n, int K, int T, int C, double* prerank, int32_t* below,
                                     int32_t* equal, int32_t* hidden, void* work, size_t work_bytes, void* stream) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, samples && truth && mask_u8 && prerank && below && equal && work, "fd_multivariate_ranks: null pointer");
    Plan p;
    if (int rc = plan_for(ctx, "fd_multivariate_ranks", kind, n, K, T, C, &p)) return rc;
    FD_REQUIRE(ctx, work_bytes >= p.bytes, "fd_multivariate_ranks: workspace of %zu bytes, needs %zu", work_bytes, p.bytes);
    hipStream_t st = (hipStream_t)stream;
    const int per = mask_per_series ? 1 : 0;
    const dim3 block(kThreads);
    long long* part = (long long*)work;
    if (kind == FD_PRERANK_MST) {
        double* dist = (double*)work;
        int32_t* flags = (int32_t*)((char*)work + p.flag_offset);
        const int nflag = p.ntile * p.ntile;
        hipLaunchKernelGGL(k_tiles<false>, dim3((unsigned)(n * nflag)), block, 0, st, samples, truth, mask_u8, per, K, p.TC, p.ntile,
                           (long long*)nullptr, dist, flags);
        FD_LAUNCH_CHECK(ctx);
        const int pt = p.m <= 64 ? 64 : p.m <= 128 ? 128 : kThreads;
        hipLaunchKernelGGL(k_prim, dim3((unsigned)(n * p.m)), dim3(pt), 0, st, dist, p.m, prerank);
        FD_LAUNCH_CHECK(ctx);
        hipLaunchKernelGGL(k_rank_finish, dim3((unsigned)n), block, 0, st, 1, (const long long*)nullptr, 0, nflag, flags, p.m, p.TC,
                           mask_u8, per, prerank, below, equal, hidden);
        FD_LAUNCH_CHECK(ctx);
        return FD_OK;
    }
    int P, nflag;
    if (kind == FD_PRERANK_DOMINANCE) {
        P = p.ntile;
        nflag = p.ntile;
        hipLaunchKernelGGL(k_tiles<true>, dim3((unsigned)(n * p.ntile * p.ntile)), block, 0, st, samples, truth, mask_u8, per, K,
                           p.TC, p.ntile, part, (double*)nullptr, (int32_t*)nullptr);
    } else {
        P = p.S;
        nflag = 1;
        if (kind == FD_PRERANK_AVERAGE)
            hipLaunchKernelGGL(k_count<FD_PRERANK_AVERAGE>, dim3((unsigned)(n * p.S)), block, 0, st, samples, truth, mask_u8, per, K,
                               p.TC, p.S, part);
        else
            hipLaunchKernelGGL(k_count<FD_PRERANK_BAND_DEPTH>, dim3((unsigned)(n * p.S)), block, 0, st, samples, truth, mask_u8, per,
                               K, p.TC, p.S, part);
    }
    FD_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_rank_finish, dim3((unsigned)n), block, 0, st, 0, part, P, nflag, (const int32_t*)nullptr, p.m, p.TC, mask_u8,
                       per, prerank, below, equal, hidden);
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}
