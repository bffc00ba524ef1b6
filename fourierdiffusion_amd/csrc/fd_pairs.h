// fd_pairs.h -- what the all-pairs metric kernels share: fd_neighbours.hip (k_nn), fd_mmd.hip (k_mmd),
// fd_dtw.hip (k_dtw) and fd_sinkhorn.hip (k_softmin) include it; every piece below exists once.
//
//   k-best list     KBest<KMAX> under the strict (distance, index) order, the merge of the splits' lists (k_merge_lists, its
//                   output written by the caller's tail) and the sum of the splits' counts (sum_counts): k_nn and k_dtw.
//   centring        column mean of a row set (double partial sums in a fixed order) and the centred, padded copy with its row
//                   norms (centre_mean, centre_rows); the double-precision mean and deviations are an option: k_nn, k_mmd and k_softmin.
//                   These and sum_counts are plain kernels, compiled once in fd_pairs.hip.
//   Gram tiles      FD_GRAM_TILES_BEGIN / _END: a workgroup of 256 threads OWNS 128 rows (the columns of D) and STREAMS 128-row
//                   tiles of a second set (the rows of D), 16 features at a time, double-buffered through the LDS into
//                   v_mfma_f32_32x32x2_f32; every finished 128 x 128 accumulator tile goes to the caller's epilogue.
//                   FD_GRAM_ROW / FD_GRAM_DRAIN are the only place that knows which accumulator register is which row: k_nn,
//                   k_mmd and k_softmin.
//   planning        plan_splits (forced count or fill the device, clamped, whole units per split) and Carve (offsets of a
//                   256-byte-aligned workspace).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>

#include "fd_common.h"

namespace fdp {

constexpr int TQ = 128, TR = 128, KC = 16, NT = 256, LDW = 128 + 4;
constexpr int MEAN_ROWS = 512;       // rows per partial column sum
constexpr int MAX_SPLITS = 64;
constexpr int MAX_K = 16;
typedef float f32x16 __attribute__((ext_vector_type(16)));

// the padded shapes of the centred copies, and the chunks of the column sums
inline int padded_features(int d) { return fd_cdiv(d, KC) * KC; }
inline int padded_rows(int n) { return fd_cdiv(n, TQ) * TQ; }
inline int mean_chunks(int m) { return fd_cdiv(m, MEAN_ROWS); }

// ---------------------------------------------------------------------------------------------- fd_pairs.hip
// counts[i] = the partial counts pc (splits, n) of query i, added in split order
void sum_counts(const int* pc, int splits, int n, int32_t* counts, hipStream_t s);
// mean (padded_features(d)) [and meand, unless null] = the column mean of x (m, d): double partial sums over 512-row chunks in row
// order, the chunks in order, / m, rounded to f32; 0 in the padded columns.  part: (mean_chunks(m), d) doubles
void centre_mean(const float* x, int m, int d, double* part, double* meand, float* mean, hipStream_t s);
// xc (padded_rows(rows), padded_features(d)) = x - mean in f32, zero in the padding; norm[row] = ||xc[row]||^2 (double sum of the f32
// values' squares).  Unless null, ss[row] = ||x[row] - meand||^2 entirely in double.
void centre_rows(const float* x, int rows, int d, const float* mean, const double* meand, float* xc, float* norm, double* ss,
                 hipStream_t s);

namespace {

// ---------------------------------------------------------------------------------------------- k-best list
__device__ __forceinline__ bool before(float a, int ai, float b, int bi) { return a < b || (a == b && ai < bi); }

// KMAX (distance, index) pairs in registers, ascending; unused slots hold (+inf, INT_MAX), which nothing real comes after
template <int KMAX>
struct KBest {
    float d[KMAX];
    int i[KMAX];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int p = 0; p < KMAX; ++p) { d[p] = INFINITY; i[p] = INT_MAX; }
    }
    __device__ __forceinline__ void push(float v, int j) {
        if (!before(v, j, d[KMAX - 1], i[KMAX - 1])) return;
        d[KMAX - 1] = v;
        i[KMAX - 1] = j;
#pragma unroll
        for (int p = KMAX - 1; p > 0; --p) {
            const bool sw = before(d[p], i[p], d[p - 1], i[p - 1]);
            const float lo_d = sw ? d[p] : d[p - 1], hi_d = sw ? d[p - 1] : d[p];
            const int lo_i = sw ? i[p] : i[p - 1], hi_i = sw ? i[p - 1] : i[p];
            d[p - 1] = lo_d; d[p] = hi_d;
            i[p - 1] = lo_i; i[p] = hi_i;
        }
    }
};

// one thread per query: the k best of the splits' lists; tail(position in the (n, k) output, distance, index) writes them out (an
// empty slot arrives as (+inf, INT_MAX))
template <int KMAX, class Tail>
__global__ __launch_bounds__(256) void k_merge_lists(const float* __restrict__ pd, const int* __restrict__ pi, int splits, int n, int k,
                                                     Tail tail) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    KBest<KMAX> best;
    best.init();
    for (int z = 0; z < splits; ++z) {
        const size_t o = ((size_t)z * n + i) * KMAX;
#pragma unroll
        for (int p = 0; p < KMAX; ++p) best.push(pd[o + p], pi[o + p]);
    }
#pragma unroll
    for (int p = 0; p < KMAX; ++p)
        if (p < k) tail((size_t)i * k + p, best.d[p], best.i[p]);
}

template <int KMAX, class Tail>
void merge_lists(const float* pd, const int* pi, int splits, int n, int k, Tail tail, hipStream_t s) {
    hipLaunchKernelGGL((k_merge_lists<KMAX, Tail>), dim3(fd_cdiv(n, 256)), dim3(256), 0, s, pd, pi, splits, n, k, tail);
}

// ---------------------------------------------------------------------------------------------- Gram tiles
// The D layout of v_mfma_f32_32x32x2_f32 as the tile loop uses it: the column of D is the lane's owned row 32 wave + (lane & 31);
// register i of accumulator t is streamed row FD_GRAM_ROW(0, t, i, lane >> 5) of the tile; base is added first.  (half = 0: the
// part every lane shares; the rest, 4 (lane >> 5), can then sit in a base pointer.)
#define FD_GRAM_ROW(base, t, i, half) ((base) + 32 * (t) + 8 * ((i) >> 2) + 4 * (half) + ((i) & 3))

// FD_GRAM_ACC(acc); the accumulators of the tile loop, cleared
#define FD_GRAM_ACC(acc)                          \
    f32x16 acc[4];                                \
    _Pragma("unroll") for (int t = 0; t < 4; ++t) \
        _Pragma("unroll") for (int i = 0; i < 16; ++i) acc[t][i] = 0.f

// FD_GRAM_DRAIN(t, i) STATEMENT: the statement for the 64 registers acc[t][i] of a finished tile, in ascending (t, i); it clears them
#define FD_GRAM_DRAIN(t, i) _Pragma("unroll") for (int t = 0; t < 4; ++t) _Pragma("unroll") for (int i = 0; i < 16; ++i)

// FD_GRAM_TILES_BEGIN(...) epilogue statements FD_GRAM_TILES_END, in a kernel of NT threads: streams the tiles [tbeg, tend) of str
// (tile t: rows row0 + t TR ..) against the owned rows q0 .. q0 + TQ - 1 of own (both (rows, dp), dp a size_t, nkc = dp / KC
// chunks, whole tiles), and runs the epilogue once per finished tile with
//     tile          its index,
//     acc[4]        the 128 x 128 products (FD_GRAM_ACC(acc) of the kernel; D layout above; the epilogue leaves them cleared),
//     aux[tile & 1] AUX <= 2 rows of per-streamed-row values that travelled with the tile (||r||^2, a radius ...): the trailing macro
//                   arguments are the statements that fetch ra0 (and, with USED = 2, ra1) of streamed row j (threads tid < TR).
// It declares the LDS (two 16 x 128 feature tiles and aux, double-buffered by tile parity: aux of a parity is rewritten two tiles
// on, behind a barrier every wave passes after the epilogue); the kernel has tid, lane = tid & 63 and wave = tid >> 6.
// This is text and not a device template on purpose: a template is optimised on its own before it is inlined, with the caller's
// state behind references, and the kernels that came out of that differed from the hand-written ones (k_nn<16> 229 instead of 254
// VGPRs).  Expanded in place the loop is part of the kernel's body from the start; the kernel declares acc, nkc
// and dp itself because even the order of those statements shows in the generated code.
#define FD_GRAM_TILES_BEGIN(AUX, USED, own, str, dp, nkc, q0, row0, tbeg, tend, ...)                                                   \
    __shared__ float Qs[KC][LDW];                                                                                                      \
    __shared__ float Rs[KC][LDW];                                                                                                      \
    __shared__ float aux[2][AUX][TR];                                                                                                  \
    const int tile_beg = (tbeg), tile_end = (tend);                                                                                    \
    /* staging: thread -> (row = id / 4, features 4 (id % 4) .. + 3) of both 128 x 16 tiles, two ids per thread */                     \
    float4 rq[2], rr[2];                                                                                                               \
    float ra0 = 0.f, ra1 = 0.f;                                                                                                        \
    auto gload = [&](int tile, int kc) {                                                                                               \
        const int j0 = (row0) + tile * TR, k0 = kc * KC;                                                                               \
        _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                                                \
            const int id = tid + i * NT, row = id >> 2, kq = id & 3;                                                                   \
            rq[i] = *reinterpret_cast<const float4*>((own) + (size_t)((q0) + row) * (dp) + k0 + 4 * kq);                                 \
            rr[i] = *reinterpret_cast<const float4*>((str) + (size_t)(j0 + row) * (dp) + k0 + 4 * kq);                                   \
        }                                                                                                                              \
        if (kc == 0 && tid < TR) {                                                                                                     \
            const int j = j0 + tid;                                                                                                    \
            __VA_ARGS__                                                                                                                \
        }                                                                                                                              \
    };                                                                                                                                 \
    auto sstore = [&](int tile, int kc) {                                                                                              \
        _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                                                \
            const int id = tid + i * NT, row = id >> 2, kq = id & 3;                                                                   \
            Qs[4 * kq + 0][row] = rq[i].x; Qs[4 * kq + 1][row] = rq[i].y; Qs[4 * kq + 2][row] = rq[i].z; Qs[4 * kq + 3][row] = rq[i].w; \
            Rs[4 * kq + 0][row] = rr[i].x; Rs[4 * kq + 1][row] = rr[i].y; Rs[4 * kq + 2][row] = rr[i].z; Rs[4 * kq + 3][row] = rr[i].w; \
        }                                                                                                                              \
        if (kc == 0 && tid < TR) {                                                                                                     \
            aux[tile & 1][0][tid] = ra0;                                                                                               \
            if ((USED) > 1) aux[tile & 1][(USED) - 1][tid] = ra1;                                                                      \
        }                                                                                                                              \
    };                                                                                                                                 \
    if (tile_beg < tile_end) gload(tile_beg, 0);                                                                                       \
    for (int tile = tile_beg; tile < tile_end; ++tile) {                                                                               \
        for (int kc = 0; kc < nkc; ++kc) {                                                                                             \
            sstore(tile, kc);                                                                                                          \
            __syncthreads();                                                                                                           \
            if (kc + 1 < nkc) gload(tile, kc + 1);                                                                                     \
            else if (tile + 1 < tile_end) gload(tile + 1, 0);                                                                          \
            /* 32x32x2: lane l holds row / column l & 31 of k-slot l >> 5; A = streamed rows (rows of D), B = owned (columns of D) */  \
            _Pragma("unroll") for (int kk = 0; kk < KC / 2; ++kk) {                                                                    \
                const int k = 2 * kk + (lane >> 5);                                                                                    \
                const float b = Qs[k][32 * wave + (lane & 31)];                                                                        \
                _Pragma("unroll") for (int t = 0; t < 4; ++t)                                                                          \
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(Rs[k][32 * t + (lane & 31)], b, acc[t], 0, 0, 0);                    \
            }                                                                                                                          \
            __syncthreads();                                                                                                           \
        }
#define FD_GRAM_TILES_END }

// ---------------------------------------------------------------------------------------------- planning
// Splits of `units` (tiles) of work: the count the environment variable `env` forces (tests), else `want` (what fills the device),
// at most MAX_SPLITS and one per unit; a split is a whole number of units.
inline void plan_splits(const char* env, int want, int units, int* splits, int* units_per_split) {
    const char* e = getenv(env);
    const int forced = e ? atoi(e) : 0;
    const int s = std::min(forced > 0 ? forced : want, std::min(units, MAX_SPLITS));
    *units_per_split = fd_cdiv(units, s);
    *splits = fd_cdiv(units, *units_per_split);
}

// offsets of the pieces of a workspace whose base the callee rounds up to 256 bytes (align)
struct Carve {
    size_t off = 0;
    size_t take(size_t bytes) { const size_t o = off; off += fd_ws::padded(bytes); return o; }
    size_t bytes() const { return off + 256; }
    static char* align(void* work) { return (char*)(((uintptr_t)work + 255) & ~(uintptr_t)255); }
};

}  // namespace
}  // namespace fdp
