// fd_neighbours.hip -- nearest-neighbour primitives of the sample-space metrics (NOT in the reference; improved precision / recall,
// density / coverage, authenticity and the train-versus-held-out share all reduce to them).
//
//   fd_knn_rows     the k nearest reference rows of every query row, sorted by (distance, index)
//   fd_ball_counts  counts[i] = #{ j : d2(q_i, r_j) <= radius2[j] }
//
// Both run one fused kernel (k_nn) over the centred expansion ||q||^2 + ||r||^2 - 2 q.r on v_mfma_f32_32x32x2_f32: the n x m
// matrix never exists.  Both sets are centred by the reference set's column mean (double sums in a fixed order) into padded
// copies, so the expansion's cancellation error scales with the spread of the data and not with its offset.
//
//   k_nn            a workgroup owns 128 queries and streams 128-row reference tiles (16 features at a time) through the LDS.  The
//                   queries sit on the MFMA's COLUMN axis: in the C/D layout a lane's 16 registers are 16 reference rows of ONE
//                   query, so wave w / lane l owns query 32 w + (l & 31) and keeps its k-best list in registers ((distance, index)
//                   pairs, sorted; an insertion is a compare against the tail and a bubble pass).  The two half-waves of a query are
//                   merged by lane exchange at the end.  gridDim.y splits the reference rows when there are too few query tiles
//                   to fill the device; every split writes its list, and k_knn_merge merges them.  Every comparison is on
//                   (distance, index), a strict total order, so the result does not depend on the split.
//   refinement      the k selected pairs are recomputed in the direct form sum (q - r)^2 on the ORIGINAL rows (f32 differences,
//                   double sum in ascending feature order) and re-sorted: a returned distance is exact to f32 rounding, and a
//                   bit-copy of a reference row returns that row with distance exactly 0.
//   counts          the same kernel with a compare-and-count epilogue; integer partial counts per split, added in split order.
//                   No atomics anywhere: two runs are bit-identical.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdlib>

#include "fd_common.h"

namespace {

constexpr int TQ = 128, TR = 128, KC = 16, NT = 256, LDW = 128 + 4;
constexpr int MEAN_ROWS = 512;       // rows per partial column sum
constexpr int MAX_SPLITS = 64;
constexpr int MAX_K = 16;
typedef float nn_f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------------- centring
// partial column sums in double: block b = (row chunk b / ncb, column block b % ncb), rows in ascending order
__global__ __launch_bounds__(256) void k_col_partial(const float* __restrict__ x, double* __restrict__ part, int m, int d, int ncb) {
    const int chunk = blockIdx.x / ncb, c = (blockIdx.x - chunk * ncb) * 256 + threadIdx.x;
    if (c >= d) return;
    const int r0 = chunk * MEAN_ROWS, r1 = min(m, r0 + MEAN_ROWS);
    double s = 0.0;
#pragma unroll 8
    for (int r = r0; r < r1; ++r) s += (double)x[(size_t)r * d + c];
    part[(size_t)chunk * d + c] = s;
}

// mean[c] = (sum of the partials in chunk order) / m, 0 in the padded columns
__global__ __launch_bounds__(256) void k_col_mean(const double* __restrict__ part, float* __restrict__ mean, int chunks, int m, int d,
                                                  int dp) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= dp) return;
    double s = 0.0;
    if (c < d)
        for (int z = 0; z < chunks; ++z) s += part[(size_t)z * d + c];
    mean[c] = (float)(s / (double)m);
}

// xc (rows_pad, dp) = x - mean, zero in the padding; norm[row] = ||xc[row]||^2 (double sum of the f32 values' squares, one wave per row)
__global__ __launch_bounds__(256) void k_centre(const float* __restrict__ x, const float* __restrict__ mean, float* __restrict__ xc,
                                                float* __restrict__ norm, int rows, int rows_pad, int d, int dp) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows_pad) return;
    double s = 0.0;
    for (int c = lane; c < dp; c += 64) {
        float v = 0.f;
        if (row < rows && c < d) v = x[(size_t)row * d + c] - mean[c];
        xc[(size_t)row * dp + c] = v;
        s += (double)v * (double)v;
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
    if (lane == 0) norm[row] = (float)s;
}

// ---------------------------------------------------------------------------------------------- k-best list
__device__ __forceinline__ bool nn_before(float a, int ai, float b, int bi) { return a < b || (a == b && ai < bi); }

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
        if (!nn_before(v, j, d[KMAX - 1], i[KMAX - 1])) return;
        d[KMAX - 1] = v;
        i[KMAX - 1] = j;
#pragma unroll
        for (int p = KMAX - 1; p > 0; --p) {
            const bool sw = nn_before(d[p], i[p], d[p - 1], i[p - 1]);
            const float lo_d = sw ? d[p] : d[p - 1], hi_d = sw ? d[p - 1] : d[p];
            const int lo_i = sw ? i[p] : i[p - 1], hi_i = sw ? i[p - 1] : i[p];
            d[p - 1] = lo_d; d[p] = hi_d;
            i[p - 1] = lo_i; i[p] = hi_i;
        }
    }
};

// ---------------------------------------------------------------------------------------------- the fused kernel
struct NnArgs {
    const float* qc;      // (npad, dp) centred queries, npad % TQ == 0
    const float* qn;      // (npad)
    const float* rc;      // (mpad, dp) centred references, mpad % TR == 0
    const float* rn;      // (mpad)
    const float* rad2;    // (m), counts only
    int n, m, dp, rows_per_split, exclude_self;
    float* pd;            // (splits, n, KMAX) partial lists
    int* pi;
    int* pc;              // (splits, n) partial counts
};

template <int KMAX, bool COUNT>
__global__ __launch_bounds__(NT, 2) void k_nn(NnArgs g) {
    __shared__ float Qs[KC][LDW];
    __shared__ float Rs[KC][LDW];
    __shared__ float aux[2][2][TR];          // [tile parity][0: ||r||^2, 1: radius^2][row of the tile]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q0 = blockIdx.x * TQ;
    const int jbeg = blockIdx.y * g.rows_per_split, jend = min(g.m, jbeg + g.rows_per_split);
    const int ntile = (jend - jbeg + TR - 1) / TR, nkc = g.dp / KC;
    const int qi = q0 + 32 * wave + (lane & 31);            // this lane's query (< npad)
    const float qnorm = g.qn[qi];
    const size_t dp = (size_t)g.dp;

    nn_f32x16 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
    KBest<KMAX> best;
    best.init();
    int cnt = 0;

    // staging: thread -> (row = id / 4, features 4 (id % 4) .. + 3) of both 128 x 16 tiles, two ids per thread
    float4 rq[2], rr[2];
    float ra0 = 0.f, ra1 = 0.f;
    auto gload = [&](int tile, int kc) {
        const int j0 = jbeg + tile * TR, k0 = kc * KC;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int id = tid + i * NT, row = id >> 2, kq = id & 3;
            rq[i] = *reinterpret_cast<const float4*>(g.qc + (size_t)(q0 + row) * dp + k0 + 4 * kq);
            rr[i] = *reinterpret_cast<const float4*>(g.rc + (size_t)(j0 + row) * dp + k0 + 4 * kq);
        }
        if (kc == 0 && tid < TR) {
            ra0 = g.rn[j0 + tid];
            if (COUNT) ra1 = (j0 + tid < g.m) ? g.rad2[j0 + tid] : -1.f;
        }
    };
    auto sstore = [&](int tile, int kc) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int id = tid + i * NT, row = id >> 2, kq = id & 3;
            Qs[4 * kq + 0][row] = rq[i].x; Qs[4 * kq + 1][row] = rq[i].y; Qs[4 * kq + 2][row] = rq[i].z; Qs[4 * kq + 3][row] = rq[i].w;
            Rs[4 * kq + 0][row] = rr[i].x; Rs[4 * kq + 1][row] = rr[i].y; Rs[4 * kq + 2][row] = rr[i].z; Rs[4 * kq + 3][row] = rr[i].w;
        }
        if (kc == 0 && tid < TR) {
            aux[tile & 1][0][tid] = ra0;
            if (COUNT) aux[tile & 1][1][tid] = ra1;
        }
    };

    if (ntile > 0) gload(0, 0);
    for (int tile = 0; tile < ntile; ++tile) {
        for (int kc = 0; kc < nkc; ++kc) {
            sstore(tile, kc);
            __syncthreads();
            if (kc + 1 < nkc) gload(tile, kc + 1);
            else if (tile + 1 < ntile) gload(tile + 1, 0);
            // 32x32x2: lane l holds row / column l & 31 of k-slot l >> 5; A = references (rows of D), B = queries (columns of D)
#pragma unroll
            for (int kk = 0; kk < KC / 2; ++kk) {
                const int k = 2 * kk + (lane >> 5);
                const float b = Qs[k][32 * wave + (lane & 31)];
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(Rs[k][32 * t + (lane & 31)], b, acc[t], 0, 0, 0);
            }
            __syncthreads();
        }
        // D layout: register i of accumulator t -> reference row 32 t + 8 (i / 4) + 4 (lane >> 5) + (i % 4) of the tile, column =
        // this lane's query.  aux of this tile's parity is rewritten two tiles on, behind a barrier every wave passes after this.
        const int j0 = jbeg + tile * TR;
        const float* an = aux[tile & 1][0];
        const float* ar = aux[tile & 1][1];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int rl = 32 * t + 8 * (i >> 2) + 4 * (lane >> 5) + (i & 3), j = j0 + rl;
                const float v = fmaf(-2.f, acc[t][i], qnorm + an[rl]);
                acc[t][i] = 0.f;
                if (COUNT) {
                    cnt += (j < jend && v <= ar[rl]) ? 1 : 0;
                } else {
                    if (j < jend && !(g.exclude_self && j == qi)) best.push(v, j);
                }
            }
    }

    // the two half-waves hold disjoint reference rows of the same queries: the upper half hands its result to the lower one
    if (COUNT) {
        cnt += __shfl_down(cnt, 32);
        if (lane < 32 && qi < g.n) g.pc[(size_t)blockIdx.y * g.n + qi] = cnt;
    } else {
#pragma unroll
        for (int p = 0; p < KMAX; ++p) {
            const float od = __shfl_down(best.d[p], 32);
            const int oi = __shfl_down(best.i[p], 32);
            if (lane < 32) best.push(od, oi);
        }
        if (lane < 32 && qi < g.n) {
            const size_t o = ((size_t)blockIdx.y * g.n + qi) * KMAX;
#pragma unroll
            for (int p = 0; p < KMAX; ++p) { g.pd[o + p] = best.d[p]; g.pi[o + p] = best.i[p]; }
        }
    }
}

// ---------------------------------------------------------------------------------------------- merge, refinement, sort
// one thread per query: the k best of the splits' lists
template <int KMAX>
__global__ __launch_bounds__(256) void k_knn_merge(const float* __restrict__ pd, const int* __restrict__ pi, int splits, int n, int k,
                                                   int* __restrict__ idx) {
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
        if (p < k) idx[(size_t)i * k + p] = best.i[p];
}

// one thread per selected pair: sum (q - r)^2, f32 differences, double sum in ascending feature order
__global__ __launch_bounds__(256) void k_knn_refine(const float* __restrict__ q, const float* __restrict__ r, const int* __restrict__ idx,
                                                    float* __restrict__ dist2, int n, int m, int k, int d) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n * k) return;
    const int j = idx[t];
    if (j < 0 || j >= m) {              // no candidate compared below the empty slot: the inputs were not finite
        dist2[t] = INFINITY;
        return;
    }
    const float* qa = q + (size_t)(t / k) * d;
    const float* ra = r + (size_t)j * d;
    double s = 0.0;
    for (int c = 0; c < d; ++c) {
        const float df = qa[c] - ra[c];
        s += (double)df * (double)df;
    }
    dist2[t] = (float)s;
}

// one thread per query: its k refined pairs sorted by (distance, index)
template <int KMAX>
__global__ __launch_bounds__(256) void k_knn_sort(float* __restrict__ dist2, int* __restrict__ idx, int n, int k) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    KBest<KMAX> best;
    best.init();
    const size_t o = (size_t)i * k;
#pragma unroll
    for (int p = 0; p < KMAX; ++p)
        if (p < k) best.push(dist2[o + p], idx[o + p]);
#pragma unroll
    for (int p = 0; p < KMAX; ++p)
        if (p < k) { dist2[o + p] = best.d[p]; idx[o + p] = best.i[p]; }
}

__global__ __launch_bounds__(256) void k_sum_counts(const int* __restrict__ pc, int splits, int n, int32_t* __restrict__ counts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int s = 0;
    for (int z = 0; z < splits; ++z) s += pc[(size_t)z * n + i];
    counts[i] = s;
}

// ---------------------------------------------------------------------------------------------- host side
struct NnPlan {
    int dp, npad, mpad, chunks, splits, rows_per_split, kmax;
    size_t o_part, o_mean, o_rc, o_rn, o_qc, o_qn, o_pd, o_pi, bytes;
};

// splits of the reference rows: one when the query tiles fill the device, else about two workgroups per CU; FDIFF_KNN_SPLITS forces
// a count (tests).  A split is a whole number of 128-row tiles.
void nn_splits(const fd_ctx* ctx, int n, int m, int* splits, int* rows_per_split) {
    const int tq = fd_cdiv(n, TQ), tr = fd_cdiv(m, TR);
    int s = 1;
    const char* e = getenv("FDIFF_KNN_SPLITS");
    const int forced = e ? atoi(e) : 0;
    if (forced > 0) s = forced;
    else if (tq < ctx->num_cu) s = fd_cdiv(2 * ctx->num_cu, tq);
    s = std::min(s, std::min(tr, MAX_SPLITS));
    *rows_per_split = fd_cdiv(tr, s) * TR;
    *splits = fd_cdiv(m, *rows_per_split);
}

// k = 0: the plan of fd_ball_counts (partial counts instead of lists)
NnPlan nn_plan(const fd_ctx* ctx, int n, int m, int d, int k) {
    NnPlan p;
    p.dp = fd_cdiv(d, KC) * KC;
    p.npad = fd_cdiv(n, TQ) * TQ;
    p.mpad = fd_cdiv(m, TR) * TR;
    p.chunks = fd_cdiv(m, MEAN_ROWS);
    nn_splits(ctx, n, m, &p.splits, &p.rows_per_split);
    p.kmax = k <= 1 ? 1 : k <= 8 ? 8 : MAX_K;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += fd_ws::padded(bytes); return o; };
    p.o_part = take((size_t)p.chunks * d * sizeof(double));
    p.o_mean = take((size_t)p.dp * sizeof(float));
    p.o_rc = take((size_t)p.mpad * p.dp * sizeof(float));
    p.o_rn = take((size_t)p.mpad * sizeof(float));
    p.o_qc = take((size_t)p.npad * p.dp * sizeof(float));
    p.o_qn = take((size_t)p.npad * sizeof(float));
    if (k > 0) {
        p.o_pd = take((size_t)p.splits * n * p.kmax * sizeof(float));
        p.o_pi = take((size_t)p.splits * n * p.kmax * sizeof(int));
    } else {
        p.o_pd = take((size_t)p.splits * n * sizeof(int));
        p.o_pi = p.o_pd;
    }
    p.bytes = off + 256;                      // the caller's pointer is rounded up to 256 bytes
    return p;
}

// mean of r, centred copies and norms of r and (unless it is the same set) q; fills the kernel's arguments
void nn_prepare(const NnPlan& p, char* base, const float* q, int n, const float* r, int m, int d, bool same, NnArgs* g, hipStream_t s) {
    double* part = (double*)(base + p.o_part);
    float* mean = (float*)(base + p.o_mean);
    float* rc = (float*)(base + p.o_rc);
    float* rn = (float*)(base + p.o_rn);
    float* qc = same ? rc : (float*)(base + p.o_qc);
    float* qn = same ? rn : (float*)(base + p.o_qn);
    const int ncb = fd_cdiv(d, 256);
    hipLaunchKernelGGL(k_col_partial, dim3((unsigned)p.chunks * ncb), dim3(256), 0, s, r, part, m, d, ncb);
    hipLaunchKernelGGL(k_col_mean, dim3(fd_cdiv(p.dp, 256)), dim3(256), 0, s, part, mean, p.chunks, m, d, p.dp);
    hipLaunchKernelGGL(k_centre, dim3(p.mpad / 4), dim3(256), 0, s, r, mean, rc, rn, m, p.mpad, d, p.dp);
    if (!same) hipLaunchKernelGGL(k_centre, dim3(p.npad / 4), dim3(256), 0, s, q, mean, qc, qn, n, p.npad, d, p.dp);
    g->qc = qc; g->qn = qn; g->rc = rc; g->rn = rn;
    g->rad2 = nullptr;
    g->n = n; g->m = m; g->dp = p.dp; g->rows_per_split = p.rows_per_split; g->exclude_self = 0;
    g->pd = nullptr; g->pi = nullptr; g->pc = nullptr;
}

char* nn_align(void* work) { return (char*)(((uintptr_t)work + 255) & ~(uintptr_t)255); }

}  // namespace

extern "C" int fd_knn_rows_workspace_bytes(fd_ctx* ctx, int n, int m, int d, int k, size_t* bytes) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, bytes, "fd_knn_rows_workspace_bytes: null pointer");
    FD_REQUIRE(ctx, n > 0 && m > 0 && d > 0, "fd_knn_rows_workspace_bytes: bad shape n=%d m=%d d=%d", n, m, d);
    FD_REQUIRE(ctx, k >= 1 && k <= MAX_K && k <= m, "fd_knn_rows_workspace_bytes: k=%d outside [1, min(%d, m=%d)]", k, MAX_K, m);
    FD_REQUIRE(ctx, (long long)n * k < (1ll << 31) && (long long)n * d < (1ll << 31) && (long long)m * d < (1ll << 31),
               "fd_knn_rows_workspace_bytes: too large (n * k, n * d and m * d must stay below 2^31)");
    *bytes = nn_plan(ctx, n, m, d, k).bytes;
    return FD_OK;
}

extern "C" int fd_knn_rows(fd_ctx* ctx, const float* q, int n, const float* r, int m, int d, int k, int exclude_self, float* dist2,
                           int32_t* idx, void* work, size_t work_bytes, void* stream) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, q && r && dist2 && idx && work, "fd_knn_rows: null pointer");
    FD_REQUIRE(ctx, n > 0 && m > 0 && d > 0, "fd_knn_rows: bad shape n=%d m=%d d=%d", n, m, d);
    FD_REQUIRE(ctx, !exclude_self || (q == r && n == m), "fd_knn_rows: exclude_self needs q == r and n == m (n=%d m=%d)", n, m);
    FD_REQUIRE(ctx, k >= 1 && k <= MAX_K && k <= m - (exclude_self ? 1 : 0), "fd_knn_rows: k=%d outside [1, min(%d, m - exclude_self = %d)]",
               k, MAX_K, m - (exclude_self ? 1 : 0));
    FD_REQUIRE(ctx, (long long)n * k < (1ll << 31) && (long long)n * d < (1ll << 31) && (long long)m * d < (1ll << 31),
               "fd_knn_rows: too large (n * k, n * d and m * d must stay below 2^31)");
    const NnPlan p = nn_plan(ctx, n, m, d, k);
    FD_REQUIRE(ctx, work_bytes >= p.bytes, "fd_knn_rows: workspace of %zu bytes, fd_knn_rows_workspace_bytes asks for %zu", work_bytes,
               p.bytes);
    hipStream_t s = (hipStream_t)stream;
    char* base = nn_align(work);
    NnArgs g;
    nn_prepare(p, base, q, n, r, m, d, q == r && n == m, &g, s);
    g.exclude_self = exclude_self ? 1 : 0;
    g.pd = (float*)(base + p.o_pd);
    g.pi = (int*)(base + p.o_pi);
    const dim3 grid(p.npad / TQ, p.splits), gq(fd_cdiv(n, 256));
    if (p.kmax == 1) {
        hipLaunchKernelGGL((k_nn<1, false>), grid, dim3(NT), 0, s, g);
        hipLaunchKernelGGL(k_knn_merge<1>, gq, dim3(256), 0, s, g.pd, g.pi, p.splits, n, k, idx);
    } else if (p.kmax == 8) {
        hipLaunchKernelGGL((k_nn<8, false>), grid, dim3(NT), 0, s, g);
        hipLaunchKernelGGL(k_knn_merge<8>, gq, dim3(256), 0, s, g.pd, g.pi, p.splits, n, k, idx);
    } else {
        hipLaunchKernelGGL((k_nn<MAX_K, false>), grid, dim3(NT), 0, s, g);
        hipLaunchKernelGGL(k_knn_merge<MAX_K>, gq, dim3(256), 0, s, g.pd, g.pi, p.splits, n, k, idx);
    }
    hipLaunchKernelGGL(k_knn_refine, dim3(fd_cdiv((long long)n * k, 256)), dim3(256), 0, s, q, r, idx, dist2, n, m, k, d);
    if (p.kmax == 1) hipLaunchKernelGGL(k_knn_sort<1>, gq, dim3(256), 0, s, dist2, idx, n, k);
    else if (p.kmax == 8) hipLaunchKernelGGL(k_knn_sort<8>, gq, dim3(256), 0, s, dist2, idx, n, k);
    else hipLaunchKernelGGL(k_knn_sort<MAX_K>, gq, dim3(256), 0, s, dist2, idx, n, k);
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}

extern "C" int fd_ball_counts(fd_ctx* ctx, const float* q, int n, const float* r, int m, int d, const float* radius2, int32_t* counts,
                              void* stream) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, q && r && radius2 && counts, "fd_ball_counts: null pointer");
    FD_REQUIRE(ctx, n > 0 && m > 0 && d > 0, "fd_ball_counts: bad shape n=%d m=%d d=%d", n, m, d);
    FD_REQUIRE(ctx, (long long)n * d < (1ll << 31) && (long long)m * d < (1ll << 31),
               "fd_ball_counts: too large (n * d and m * d must stay below 2^31)");
    const NnPlan p = nn_plan(ctx, n, m, d, 0);
    if (int rc = fd_ws_reserve(ctx, p.bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* base = nn_align(ctx->ws);
    NnArgs g;
    nn_prepare(p, base, q, n, r, m, d, q == r && n == m, &g, s);
    g.rad2 = radius2;
    g.pc = (int*)(base + p.o_pd);
    hipLaunchKernelGGL((k_nn<1, true>), dim3(p.npad / TQ, p.splits), dim3(NT), 0, s, g);
    hipLaunchKernelGGL(k_sum_counts, dim3(fd_cdiv(n, 256)), dim3(256), 0, s, g.pc, p.splits, n, counts);
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}
