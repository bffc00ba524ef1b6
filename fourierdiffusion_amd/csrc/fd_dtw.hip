// fd_dtw.hip -- dynamic time warping under a Sakoe-Chiba band between two sets of series (NOT in the reference; the time-warp-aware
// nearest-neighbour primitives of the sample-space metrics).
//
//   fd_dtw_pairs        dist2[i] = dtw2(a_i, b_i)
//   fd_dtw_knn          the k nearest reference series of every query, sorted by (distance, index)
//   fd_dtw_ball_counts  counts[i] = #{ j : dtw2(q_i, r_j) <= radius2[j] }
//
// All three run ONE kernel (k_dtw) around ONE cell function (dtw_cell); the n x m matrix never exists.
//
//   layout     one (query, reference) pair per LANE: the 64 lanes of a wave hold 64 consecutive reference series, the query is uniform
//              across the wave.  The references are read from an image transposed once by k_dtw_image into [tile of 64][t][c][lane]
//              (rows past m are zero), so y[j][c] of all 64 lanes is one coalesced 256-byte read; the query's values are wave-uniform
//              loads (scalar registers, no vector register and no vector instruction per cell).
//   recurrence a wave walks the band in blocks of IB = 8 query rows.  Inside a block it steps over the reference index j from
//              max(0, i0 - w) to min(T - 1, i0 + IB - 1 + w); the block's column D(i0 .. i0 + IB - 1, j - 1) is eight registers, every
//              index static.  What a block hands to the next is its bottom ROW D(i0 + IB - 1, j): one LDS word per lane and j, laid
//              out [j mod ring][lane] (conflict-free: a lane only ever touches its own column of the array, so no barrier either),
//              read once and rewritten once per column step -- 2 LDS instructions per 8 cells.  ring = min(T, 2 w + IB) rows, so the
//              LDS footprint is the band's, not the series'.  A cell outside the band (or past T) gets the query value +inf: its
//              cost and therefore its D are +inf, which is exactly "absent neighbour" for min3.  The choice is a scalar select; on the
//              columns where all eight rows are inside the band (all but 2 (IB - 1) of a block's) it is not even made.
//   cell       D = fma(d_last, d_last, m (+) P),  m = min3 of the three predecessors, d_c = x_c - y_c,  P = the fma chain of
//              d_0^2 .. d_{C-2}^2 started at 0 (C = 1: D = fma(d, d, m)): per channel one subtract and one FMA, one v_min3_f32, and for
//              C > 1 one add.  A pure function of the inputs: the result does not depend on the entry point, the tiling or the split,
//              and dtw2(a, b) == dtw2(b, a) bit for bit (x - y and y - x differ in sign only, min is exact).
//   selection  per-lane k-best lists in registers over the tiles a wave visits ((distance, index) pairs, sorted: KBest of
//              fd_pairs.h, which also has the merge, the count sum and the split planning; fd_neighbours.hip uses the same), merged
//              across the lanes by six rounds of lane exchange.  gridDim.y splits the reference tiles when the queries alone do not
//              fill the device (FDIFF_DTW_SPLITS forces a count); every split writes its list and k_merge_lists (DtwTail) merges them.  Every
//              comparison is on (distance, index), a strict total order: the result does not depend on the split.  Ball counts are
//              integer partials added in split order.  No atomics anywhere: two runs are bit-identical.
//   pairs      the same kernel with one useful lane per wave (the pair's row of b in its tile): n pairs cost what a search against
//              64 references costs, and the value is by construction the one fd_dtw_knn returns for that pair.
#include <type_traits>

#include "fd_pairs.h"

namespace {
using namespace fdp;

constexpr int LANES = 64;
#ifndef FD_DTW_IB
#define FD_DTW_IB 8
#endif
constexpr int IB = FD_DTW_IB;         // query rows of a block (the register column); the macro is for ablation builds
constexpr int MAX_T = 1024;
constexpr int MAX_BAND = 256;         // largest stored band column min(2 w + 1, T)
constexpr int DTW_KNN = 0, DTW_COUNT = 1, DTW_PAIRS = 2;

// ---------------------------------------------------------------------------------------------- the cell
// m: min of the three predecessors; partial: the cost of the channels before the last (unused when ONE); d: the last channel's difference
template <bool ONE>
__device__ __forceinline__ float dtw_cell(float m, float partial, float d) {
    return fmaf(d, d, ONE ? m : m + partial);
}

__device__ __forceinline__ float dtw_min3(float a, float b, float c) { return fminf(fminf(a, b), c); }

// dtw2 of the wave-uniform query x (T, C) against this lane's reference y (image pointer already offset by the tile and the lane;
// y[(j C + c) 64]).  row: this lane's column of the LDS ring (row[p 64], p < ring).
template <bool ONE>
__device__ __forceinline__ float dtw_tile(const float* __restrict__ x, const float* __restrict__ y, float* row, int T, int C, int w,
                                          int ring) {
    float result = INFINITY;
    for (int i0 = 0; i0 < T; i0 += IB) {
        const int jlo = max(0, i0 - w), jhi = min(T - 1, i0 + IB - 1 + w);
        int pos = jlo % ring;                                  // ring position of column j, kept by increment
        float left[IB];                                        // D(i0 + ii, j - 1): absent or outside the band at j = jlo
        float xs[IB];                                          // ONE: the block's query values (wave-uniform)
#pragma unroll
        for (int ii = 0; ii < IB; ++ii) {
            left[ii] = INFINITY;
            xs[ii] = ONE ? x[min(i0 + ii, T - 1)] : 0.f;
        }
        // D(i0 - 1, jlo - 1): the virtual corner D(-1, -1) = 0 of the first block, the previous block's bottom row otherwise
        float diag = INFINITY;
        if (i0 == 0) diag = 0.f;
        else if (jlo > 0) diag = row[(pos == 0 ? ring - 1 : pos - 1) * LANES];

        // what the next column reads from memory is fetched a column (the LDS word) or two (the reference value) ahead, so that
        // its latency lies behind the cells of the columns in between
        float ynext = ONE ? y[(size_t)jlo * LANES] : 0.f, ynext2 = ONE ? y[(size_t)min(jlo + 1, T - 1) * LANES] : 0.f;
        float upnext = INFINITY;                               // D(i0 - 1, jlo): inside the band of row i0 - 1 up to j = i0 - 1 + w
        if (i0 > 0 && jlo <= i0 - 1 + w) upnext = row[pos * LANES];

        auto column = [&](int j, auto masked) {
            constexpr bool MASK = decltype(masked)::value;
            const float up = upnext;                           // D(i0 - 1, j)
            const int npos = pos + 1 == ring ? 0 : pos + 1;
            upnext = INFINITY;                                 // (position npos is the previous block's until this block's column j + 1 writes it)
            if (i0 > 0 && j + 1 <= i0 - 1 + w && j + 1 <= jhi) upnext = row[npos * LANES];
            float partial[IB];
            if (!ONE) {
#pragma unroll
                for (int ii = 0; ii < IB; ++ii) partial[ii] = 0.f;
                for (int c = 0; c < C - 1; ++c) {
                    const float yv = y[((size_t)j * C + c) * LANES];
#pragma unroll
                    for (int ii = 0; ii < IB; ++ii) {
                        const float d = x[(size_t)min(i0 + ii, T - 1) * C + c] - yv;
                        partial[ii] = fmaf(d, d, partial[ii]);
                    }
                }
            }
            const float yl = ONE ? ynext : y[((size_t)j * C + (C - 1)) * LANES];
            // bit ii: row i0 + ii is below T and inside the band at column j, i.e. max(0, j - w - i0) <= ii <= min(IB - 1, j + w - i0, T - 1 - i0)
            unsigned rows_in = ~0u;
            if (MASK) {
                const int lo = max(0, j - w - i0), hi = min(min(IB - 1, j + w - i0), T - 1 - i0);
                rows_in = hi >= lo ? ((2u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
            }
            if (ONE) { ynext = ynext2; ynext2 = y[(size_t)min(j + 2, T - 1) * LANES]; }
            float dg = diag, u = up;
#pragma unroll
            for (int ii = 0; ii < IB; ++ii) {
                const int i = i0 + ii;
                const bool inband = (rows_in >> ii) & 1u;
                float xl = ONE ? xs[ii] : x[(size_t)min(i, T - 1) * C + (C - 1)];
                float p = ONE ? 0.f : partial[ii];
                if (MASK) {
                    // (the select is on the bit pattern: wave-uniform integers stay in scalar registers)
                    if (ONE) xl = __int_as_float(inband ? __float_as_int(xl) : 0x7f800000);
                    else p = inband ? p : INFINITY;
                }
                const float v = dtw_cell<ONE>(dtw_min3(left[ii], dg, u), p, xl - yl);
                dg = left[ii];
                left[ii] = v;
                u = v;
            }
            diag = up;
            row[pos * LANES] = left[IB - 1];                   // D(i0 + IB - 1, j), the next block's `up`
            pos = npos;
        };

        // columns [f0, f1]: all IB rows inside the band and below T, no select; the up to IB - 1 columns on either side are masked
        int f0 = jhi + 1, f1 = jhi;
        if (i0 + IB <= T && max(jlo, i0 + IB - 1 - w) <= min(jhi, i0 + w)) { f0 = max(jlo, i0 + IB - 1 - w); f1 = min(jhi, i0 + w); }
        for (int j = jlo; j < f0; ++j) column(j, std::true_type{});
#pragma unroll 2
        for (int j = f0; j <= f1; ++j) column(j, std::false_type{});
        for (int j = f1 + 1; j <= jhi; ++j) column(j, std::true_type{});
        if (i0 + IB >= T) {
#pragma unroll
            for (int ii = 0; ii < IB; ++ii)
                if (ii == T - 1 - i0) result = left[ii];
        }
    }
    return result;
}

// ---------------------------------------------------------------------------------------------- kernels
// img[((tile T + t) C + c) 64 + lane] = r[tile 64 + lane][t][c], 0 past row m
__global__ __launch_bounds__(256) void k_dtw_image(const float* __restrict__ r, float* __restrict__ img, int m, int T, int C,
                                                   size_t total) {
    const size_t d = (size_t)T * C;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const int lane = (int)(e % LANES);
        const size_t rest = e / LANES, tile = rest / d, tc = rest - tile * d;
        const size_t rowi = tile * LANES + lane;
        img[e] = rowi < (size_t)m ? r[rowi * d + tc] : 0.f;
    }
}

struct DtwArgs {
    const float* q;       // (n, T, C) queries, row-major
    const float* img;     // the references' transposed image
    const float* rad2;    // (m), counts only
    int n, m, T, C, w, ring, ntiles, tiles_per_split, exclude_self;
    float* pd;            // (splits, n, KMAX) partial lists
    int* pi;
    int* pc;              // (splits, n) partial counts
    float* out;           // (n), pairs only
};

// one wave per (query, split of the reference tiles)
template <bool ONE, int MODE, int KMAX>
__global__ __launch_bounds__(LANES) void k_dtw(DtwArgs g) {
    extern __shared__ float dtw_ring[];                       // [ring][64]
    const int lane = threadIdx.x, qi = blockIdx.x;
    const float* x = g.q + (size_t)qi * g.T * g.C;
    float* row = dtw_ring + lane;
    const size_t tile_floats = (size_t)g.T * g.C * LANES;
    int t0, t1;
    if (MODE == DTW_PAIRS) { t0 = qi / LANES; t1 = t0 + 1; }
    else { t0 = blockIdx.y * g.tiles_per_split; t1 = min(g.ntiles, t0 + g.tiles_per_split); }

    KBest<KMAX> best;
    best.init();
    int cnt = 0;
    for (int tile = t0; tile < t1; ++tile) {
        const float v = dtw_tile<ONE>(x, g.img + (size_t)tile * tile_floats + lane, row, g.T, g.C, g.w, g.ring);
        const int j = tile * LANES + lane;
        if (MODE == DTW_PAIRS) {
            if (j == qi) g.out[qi] = v;
        } else if (MODE == DTW_COUNT) {
            if (j < g.m) cnt += v <= g.rad2[j] ? 1 : 0;
        } else {
            if (j < g.m && !(g.exclude_self && j == qi)) best.push(v, j);
        }
    }
    if (MODE == DTW_COUNT) {
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o);
        if (lane == 0) g.pc[(size_t)blockIdx.y * g.n + qi] = cnt;
    } else if (MODE == DTW_KNN) {
        // the lanes hold disjoint reference rows: lane l takes lane l + o's list, o = 32 .. 1; lane 0 ends with the wave's
        for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
            for (int p = 0; p < KMAX; ++p) {
                const float od = __shfl_down(best.d[p], o);
                const int oi = __shfl_down(best.i[p], o);
                if (lane < o) best.push(od, oi);
            }
        }
        if (lane == 0) {
            const size_t o = ((size_t)blockIdx.y * g.n + qi) * KMAX;
#pragma unroll
            for (int p = 0; p < KMAX; ++p) { g.pd[o + p] = best.d[p]; g.pi[o + p] = best.i[p]; }
        }
    }
}

// the tail of the merge: distances and indices; an empty slot (the inputs were not finite) is index -1
struct DtwTail {
    float* dist2;
    int32_t* idx;
    __device__ void operator()(size_t o, float d, int j) const {
        dist2[o] = d;
        idx[o] = j == INT_MAX ? -1 : j;
    }
};

// ---------------------------------------------------------------------------------------------- host side
struct DtwPlan {
    int ntiles, splits, tiles_per_split, ring, kmax;
    size_t lds, image_floats, o_img, o_pd, o_pi, bytes;
};

// Splits of the reference tiles: one when the queries fill the device (a wave per query, about eight waves per CU), else enough to;
// FDIFF_DTW_SPLITS forces a count (tests).  k = 0: counts (integer partials); pairs: m = n, one tile per wave, no partials
DtwPlan dtw_plan(const fd_ctx* ctx, int n, int m, int T, int C, int w, int k, bool pairs) {
    DtwPlan p;
    p.ntiles = fd_cdiv(m, LANES);
    if (pairs) { p.splits = 1; p.tiles_per_split = 1; }
    else plan_splits("FDIFF_DTW_SPLITS", n < 8 * ctx->num_cu ? fd_cdiv(8 * ctx->num_cu, n) : 1, p.ntiles, &p.splits, &p.tiles_per_split);
    p.ring = std::min(T, 2 * w + IB);
    p.lds = (size_t)p.ring * LANES * sizeof(float);
    p.kmax = k <= 1 ? 1 : MAX_K;
    p.image_floats = (size_t)p.ntiles * LANES * T * C;
    Carve ws;
    p.o_img = ws.take(p.image_floats * sizeof(float));
    p.o_pd = p.o_pi = 0;
    if (!pairs) {
        if (k > 0) {
            p.o_pd = ws.take((size_t)p.splits * n * p.kmax * sizeof(float));
            p.o_pi = ws.take((size_t)p.splits * n * p.kmax * sizeof(int));
        } else {
            p.o_pd = ws.take((size_t)p.splits * n * sizeof(int));
        }
    }
    p.bytes = ws.bytes();
    return p;
}

// the checks every entry point shares; `who` is its name
int dtw_check(fd_ctx* ctx, const char* who, int n, int m, int T, int C, int window) {
    FD_REQUIRE(ctx, n > 0 && m > 0 && T > 0 && C > 0, "%s: bad shape n=%d m=%d T=%d C=%d", who, n, m, T, C);
    FD_REQUIRE(ctx, T <= MAX_T, "%s: bad shape T=%d above %d", who, T, MAX_T);
    FD_REQUIRE(ctx, window >= 0 && window <= T - 1, "%s: window=%d outside [0, T - 1 = %d]", who, window, T - 1);
    FD_REQUIRE(ctx, std::min(2 * window + 1, T) <= MAX_BAND, "%s: window=%d stores a band column of %d, above %d", who, window,
               std::min(2 * window + 1, T), MAX_BAND);
    const long long d = (long long)T * C;
    FD_REQUIRE(ctx, d < (1ll << 31) && (long long)n * d < (1ll << 31) && (long long)m * d < (1ll << 31),
               "%s: too large (n * T * C and m * T * C must stay below 2^31)", who);
    return FD_OK;
}

template <bool ONE, int MODE, int KMAX>
int dtw_launch_as(fd_ctx* ctx, const DtwPlan& p, const DtwArgs& g, hipStream_t s) {
    static unsigned long long attr = 0;
    if (p.lds > 64 * 1024 && fd_first_on_device(attr, ctx->device))
        FD_HIP(ctx, hipFuncSetAttribute((const void*)k_dtw<ONE, MODE, KMAX>, hipFuncAttributeMaxDynamicSharedMemorySize, 72 * 1024));
    hipLaunchKernelGGL((k_dtw<ONE, MODE, KMAX>), dim3(g.n, p.splits), dim3(LANES), p.lds, s, g);
    return FD_OK;
}

template <int MODE, int KMAX>
int dtw_launch(fd_ctx* ctx, const DtwPlan& p, const DtwArgs& g, hipStream_t s) {
    return g.C == 1 ? dtw_launch_as<true, MODE, KMAX>(ctx, p, g, s) : dtw_launch_as<false, MODE, KMAX>(ctx, p, g, s);
}

void dtw_image(const fd_ctx* ctx, const DtwPlan& p, const float* r, float* img, int m, int T, int C, hipStream_t s) {
    hipLaunchKernelGGL(k_dtw_image, dim3(fd_grid_for(p.image_floats, 256, ctx->num_cu)), dim3(256), 0, s, r, img, m, T, C,
                       p.image_floats);
}

DtwArgs dtw_args(const DtwPlan& p, const float* q, const float* img, int n, int m, int T, int C, int w) {
    DtwArgs g;
    g.q = q; g.img = img; g.rad2 = nullptr;
    g.n = n; g.m = m; g.T = T; g.C = C; g.w = w; g.ring = p.ring; g.ntiles = p.ntiles; g.tiles_per_split = p.tiles_per_split;
    g.exclude_self = 0;
    g.pd = nullptr; g.pi = nullptr; g.pc = nullptr; g.out = nullptr;
    return g;
}

}  // namespace

extern "C" int fd_dtw_pairs(fd_ctx* ctx, const float* a, const float* b, int n, int T, int C, int window, float* dist2, void* stream) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, a && b && dist2, "fd_dtw_pairs: null pointer");
    if (int rc = dtw_check(ctx, "fd_dtw_pairs", n, n, T, C, window)) return rc;
    const DtwPlan p = dtw_plan(ctx, n, n, T, C, window, 0, true);
    if (int rc = fd_ws_reserve(ctx, p.bytes)) return rc;
    ++ctx->ws_gen;
    hipStream_t s = (hipStream_t)stream;
    float* img = (float*)(Carve::align(ctx->ws) + p.o_img);
    dtw_image(ctx, p, b, img, n, T, C, s);
    DtwArgs g = dtw_args(p, a, img, n, n, T, C, window);
    g.out = dist2;
    if (int rc = dtw_launch<DTW_PAIRS, 1>(ctx, p, g, s)) return rc;
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}

extern "C" int fd_dtw_knn_workspace_bytes(fd_ctx* ctx, int n, int m, int T, int C, int window, int k, size_t* bytes) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, bytes, "fd_dtw_knn_workspace_bytes: null pointer");
    if (int rc = dtw_check(ctx, "fd_dtw_knn_workspace_bytes", n, m, T, C, window)) return rc;
    FD_REQUIRE(ctx, k >= 1 && k <= MAX_K && k <= m, "fd_dtw_knn_workspace_bytes: k=%d outside [1, min(%d, m=%d)]", k, MAX_K, m);
    FD_REQUIRE(ctx, (long long)n * k < (1ll << 31), "fd_dtw_knn_workspace_bytes: too large (n * k must stay below 2^31)");
    *bytes = dtw_plan(ctx, n, m, T, C, window, k, false).bytes;
    return FD_OK;
}

extern "C" int fd_dtw_knn(fd_ctx* ctx, const float* q, int n, const float* r, int m, int T, int C, int window, int k, int exclude_self,
                          float* dist2, int32_t* idx, void* work, size_t work_bytes, void* stream) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, q && r && dist2 && idx && work, "fd_dtw_knn: null pointer");
    if (int rc = dtw_check(ctx, "fd_dtw_knn", n, m, T, C, window)) return rc;
    FD_REQUIRE(ctx, !exclude_self || (q == r && n == m), "fd_dtw_knn: exclude_self needs q == r and n == m (n=%d m=%d)", n, m);
    FD_REQUIRE(ctx, k >= 1 && k <= MAX_K && k <= m - (exclude_self ? 1 : 0), "fd_dtw_knn: k=%d outside [1, min(%d, m - exclude_self = %d)]",
               k, MAX_K, m - (exclude_self ? 1 : 0));
    FD_REQUIRE(ctx, (long long)n * k < (1ll << 31), "fd_dtw_knn: too large (n * k must stay below 2^31)");
    const DtwPlan p = dtw_plan(ctx, n, m, T, C, window, k, false);
    FD_REQUIRE(ctx, work_bytes >= p.bytes, "fd_dtw_knn: workspace of %zu bytes, fd_dtw_knn_workspace_bytes asks for %zu", work_bytes,
               p.bytes);
    hipStream_t s = (hipStream_t)stream;
    char* base = Carve::align(work);
    float* img = (float*)(base + p.o_img);
    dtw_image(ctx, p, r, img, m, T, C, s);
    DtwArgs g = dtw_args(p, q, img, n, m, T, C, window);
    g.exclude_self = exclude_self ? 1 : 0;
    g.pd = (float*)(base + p.o_pd);
    g.pi = (int*)(base + p.o_pi);
    if (p.kmax == 1) {
        if (int rc = dtw_launch<DTW_KNN, 1>(ctx, p, g, s)) return rc;
        merge_lists<1>(g.pd, g.pi, p.splits, n, k, DtwTail{dist2, idx}, s);
    } else {
        if (int rc = dtw_launch<DTW_KNN, MAX_K>(ctx, p, g, s)) return rc;
        merge_lists<MAX_K>(g.pd, g.pi, p.splits, n, k, DtwTail{dist2, idx}, s);
    }
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}

extern "C" int fd_dtw_ball_counts_workspace_bytes(fd_ctx* ctx, int n, int m, int T, int C, int window, size_t* bytes) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, bytes, "fd_dtw_ball_counts_workspace_bytes: null pointer");
    if (int rc = dtw_check(ctx, "fd_dtw_ball_counts_workspace_bytes", n, m, T, C, window)) return rc;
    *bytes = dtw_plan(ctx, n, m, T, C, window, 0, false).bytes;
    return FD_OK;
}

extern "C" int fd_dtw_ball_counts(fd_ctx* ctx, const float* q, int n, const float* r, int m, int T, int C, int window,
                                  const float* radius2, int32_t* counts, void* work, size_t work_bytes, void* stream) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, q && r && radius2 && counts && work, "fd_dtw_ball_counts: null pointer");
    if (int rc = dtw_check(ctx, "fd_dtw_ball_counts", n, m, T, C, window)) return rc;
    const DtwPlan p = dtw_plan(ctx, n, m, T, C, window, 0, false);
    FD_REQUIRE(ctx, work_bytes >= p.bytes, "fd_dtw_ball_counts: workspace of %zu bytes, fd_dtw_ball_counts_workspace_bytes asks for %zu",
               work_bytes, p.bytes);
    hipStream_t s = (hipStream_t)stream;
    char* base = Carve::align(work);
    float* img = (float*)(base + p.o_img);
    dtw_image(ctx, p, r, img, m, T, C, s);
    DtwArgs g = dtw_args(p, q, img, n, m, T, C, window);
    g.rad2 = radius2;
    g.pc = (int*)(base + p.o_pd);
    if (int rc = dtw_launch<DTW_COUNT, 1>(ctx, p, g, s)) return rc;
    sum_counts(g.pc, p.splits, n, counts, s);
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}
