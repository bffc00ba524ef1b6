// fd_neighbours.hip -- nearest-neighbour primitives of the sample-space metrics (NOT in the reference; improved precision / recall,
// density / coverage, authenticity and the train-versus-held-out share all reduce to them).
//
//   fd_knn_rows     the k nearest reference rows of every query row, sorted by (distance, index)
//   fd_ball_counts  counts[i] = #{ j : d2(q_i, r_j) <= radius2[j] }
//
// Both run one fused kernel (k_nn) over the centred expansion ||q||^2 + ||r||^2 - 2 q.r on v_mfma_f32_32x32x2_f32: the n x m
// matrix never exists.  Both sets are centred by the reference set's column mean (double sums in a fixed order) into padded
// copies, so the expansion's cancellation error scales with the spread of the data and not with its offset.
// This file holds k_nn's epilogues, the refinement and the plan.  The centring kernels, the tile loop (LDS tiles, staging, MFMA),
// the k-best list with the merge of the splits, the count sum and the split / workspace planning are fd_pairs.h's, shared with
// fd_mmd.hip and fd_dtw.hip.
//
//   k_nn            a workgroup owns 128 queries and streams 128-row reference tiles (16 features at a time) through the LDS.  The
//                   queries sit on the MFMA's COLUMN axis: in the C/D layout a lane's 16 registers are 16 reference rows of ONE
//                   query, so wave w / lane l owns query 32 w + (l & 31) and keeps its k-best list in registers ((distance, index)
//                   pairs, sorted; an insertion is a compare against the tail and a bubble pass).  The two half-waves of a query are
//                   merged by lane exchange at the end.  gridDim.y splits the reference rows when there are too few query tiles
//                   to fill the device; every split writes its list, and k_merge_lists (KnnTail) merges them.  Every comparison is on
//                   (distance, index), a strict total order, so the result does not depend on the split.
//   refinement      the k selected pairs are recomputed in the direct form sum (q - r)^2 on the ORIGINAL rows (f32 differences,
//                   double sum in ascending feature order) and re-sorted: a returned distance is exact to f32 rounding, and a
//                   bit-copy of a reference row returns that row with distance exactly 0.
//   counts          the same kernel with a compare-and-count epilogue; integer partial counts per split, added in split order.
//                   No atomics anywhere: two runs are bit-identical.
#include <hip/hip_runtime.h>

#include "fd_pairs.h"

namespace {
using namespace fdp;

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
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q0 = blockIdx.x * TQ;
    const int jbeg = blockIdx.y * g.rows_per_split, jend = min(g.m, jbeg + g.rows_per_split);
    const int ntile = (jend - jbeg + TR - 1) / TR, nkc = g.dp / KC;
    const int qi = q0 + 32 * wave + (lane & 31);            // this lane's query (< npad)
    const float qnorm = g.qn[qi];
    const size_t dp = (size_t)g.dp;
    FD_GRAM_ACC(acc);
    KBest<KMAX> best;
    best.init();
    int cnt = 0;

    // aux: [0: ||r||^2, 1: radius^2 (counts only)]
    FD_GRAM_TILES_BEGIN(2, (COUNT ? 2 : 1), g.qc, g.rc, dp, nkc, q0, jbeg, 0, ntile,
                        ra0 = g.rn[j];
                        if (COUNT) ra1 = (j < g.m) ? g.rad2[j] : -1.f;)
        const int j0 = jbeg + tile * TR;
        const float* an = aux[tile & 1][0];
        const float* ar = aux[tile & 1][1];
        FD_GRAM_DRAIN(t, i) {
            const int rl = FD_GRAM_ROW(0, t, i, lane >> 5), j = j0 + rl;
            const float v = fmaf(-2.f, acc[t][i], qnorm + an[rl]);
            acc[t][i] = 0.f;
            if (COUNT) {
                cnt += (j < jend && v <= ar[rl]) ? 1 : 0;
            } else {
                if (j < jend && !(g.exclude_self && j == qi)) best.push(v, j);
            }
        }
    FD_GRAM_TILES_END

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
// the tail of the merge: the indices only (the distances are recomputed); an empty slot stays INT_MAX, which k_knn_refine reads as
// "no candidate"
struct KnnTail {
    int* idx;
    __device__ void operator()(size_t o, float, int j) const { idx[o] = j; }
};

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

// ---------------------------------------------------------------------------------------------- host side
struct NnPlan {
    int dp, npad, mpad, splits, rows_per_split, kmax;
    size_t o_part, o_mean, o_rc, o_rn, o_qc, o_qn, o_pd, o_pi, bytes;
};

// Splits of the reference rows (whole 128-row tiles): one when the query tiles fill the device, else about two workgroups per CU;
// FDIFF_KNN_SPLITS forces a count (tests).  k = 0: the plan of fd_ball_counts (partial counts instead of lists)
NnPlan nn_plan(const fd_ctx* ctx, int n, int m, int d, int k) {
    NnPlan p;
    p.dp = padded_features(d);
    p.npad = padded_rows(n);
    p.mpad = padded_rows(m);
    const int tq = p.npad / TQ;
    int tiles_per_split;
    plan_splits("FDIFF_KNN_SPLITS", tq < ctx->num_cu ? fd_cdiv(2 * ctx->num_cu, tq) : 1, p.mpad / TR, &p.splits, &tiles_per_split);
    p.rows_per_split = tiles_per_split * TR;
    p.kmax = k <= 1 ? 1 : k <= 8 ? 8 : MAX_K;
    Carve ws;
    p.o_part = ws.take((size_t)mean_chunks(m) * d * sizeof(double));
    p.o_mean = ws.take((size_t)p.dp * sizeof(float));
    p.o_rc = ws.take((size_t)p.mpad * p.dp * sizeof(float));
    p.o_rn = ws.take((size_t)p.mpad * sizeof(float));
    p.o_qc = ws.take((size_t)p.npad * p.dp * sizeof(float));
    p.o_qn = ws.take((size_t)p.npad * sizeof(float));
    if (k > 0) {
        p.o_pd = ws.take((size_t)p.splits * n * p.kmax * sizeof(float));
        p.o_pi = ws.take((size_t)p.splits * n * p.kmax * sizeof(int));
    } else {
        p.o_pd = ws.take((size_t)p.splits * n * sizeof(int));
        p.o_pi = p.o_pd;
    }
    p.bytes = ws.bytes();
    return p;
}

// mean of r, centred copies and norms of r and (unless it is the same set) q; fills the kernel's arguments
void nn_prepare(const NnPlan& p, char* base, const float* q, int n, const float* r, int m, int d, bool same, NnArgs* g, hipStream_t s) {
    float* mean = (float*)(base + p.o_mean);
    float* rc = (float*)(base + p.o_rc);
    float* rn = (float*)(base + p.o_rn);
    float* qc = same ? rc : (float*)(base + p.o_qc);
    float* qn = same ? rn : (float*)(base + p.o_qn);
    centre_mean(r, m, d, (double*)(base + p.o_part), nullptr, mean, s);
    centre_rows(r, m, d, mean, nullptr, rc, rn, nullptr, s);
    if (!same) centre_rows(q, n, d, mean, nullptr, qc, qn, nullptr, s);
    g->qc = qc; g->qn = qn; g->rc = rc; g->rn = rn;
    g->rad2 = nullptr;
    g->n = n; g->m = m; g->dp = p.dp; g->rows_per_split = p.rows_per_split; g->exclude_self = 0;
    g->pd = nullptr; g->pi = nullptr; g->pc = nullptr;
}

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
    char* base = Carve::align(work);
    NnArgs g;
    nn_prepare(p, base, q, n, r, m, d, q == r && n == m, &g, s);
    g.exclude_self = exclude_self ? 1 : 0;
    g.pd = (float*)(base + p.o_pd);
    g.pi = (int*)(base + p.o_pi);
    const dim3 grid(p.npad / TQ, p.splits), gq(fd_cdiv(n, 256));
    if (p.kmax == 1) {
        hipLaunchKernelGGL((k_nn<1, false>), grid, dim3(NT), 0, s, g);
        merge_lists<1>(g.pd, g.pi, p.splits, n, k, KnnTail{idx}, s);
    } else if (p.kmax == 8) {
        hipLaunchKernelGGL((k_nn<8, false>), grid, dim3(NT), 0, s, g);
        merge_lists<8>(g.pd, g.pi, p.splits, n, k, KnnTail{idx}, s);
    } else {
        hipLaunchKernelGGL((k_nn<MAX_K, false>), grid, dim3(NT), 0, s, g);
        merge_lists<MAX_K>(g.pd, g.pi, p.splits, n, k, KnnTail{idx}, s);
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
    char* base = Carve::align(ctx->ws);
    NnArgs g;
    nn_prepare(p, base, q, n, r, m, d, q == r && n == m, &g, s);
    g.rad2 = radius2;
    g.pc = (int*)(base + p.o_pd);
    hipLaunchKernelGGL((k_nn<1, true>), dim3(p.npad / TQ, p.splits), dim3(NT), 0, s, g);
    sum_counts(g.pc, p.splits, n, counts, s);
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}
