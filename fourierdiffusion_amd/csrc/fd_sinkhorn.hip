// fd_sinkhorn.hip -- entropic optimal transport between two sample sets (NOT in the reference; Genevay et al. 2018, Feydy et al.
// 2019): the soft-min pass of the Sinkhorn iteration and the whole iteration, cost ||x - y||^2.
//
//   fd_softmin_pairs        out_i = -eps log sum_j exp((h_j - ||x_i - y_j||^2) / eps) for every row of x: one pass
//   fd_sinkhorn_potentials  the dual potentials (f, g) after n_steps iterations under a schedule of eps, all enqueued on the stream;
//                           the debiased divergence is host arithmetic on three such calls (utils/sinkhorn.py)
//
// One fused kernel (k_softmin): the n x m matrix never exists.  It is a third epilogue of fd_pairs.h's tile loop, next to k_nn's
// k-best list and k_mmd's second product; the centring, the tile loop and the planning are fd_pairs.h's.
//
//   distances       both sets are centred by the mean of the pooled rows into padded copies; a workgroup owns 128 rows of one set
//                   and streams 128-row tiles of the other; d2 = max(0, ||a||^2 + ||b||^2 - 2 a.b) on v_mfma_f32_32x32x2_f32.
//   exponent        e_ij = (h_j - d2_ij) s with s = f32(log2 e / eps): the streamed row's s h_j (double product, rounded once)
//                   and ||y_j||^2 travel with the tile as the loop's two aux rows, so e is one fma on d2.  A padded streamed row
//                   gets s h_j = -inf where the aux row is fetched, BY INDEX (j >= m): whatever the padded row holds, its term is
//                   exp2(-inf) = 0.  (After the centring a padded row sits at the mean; for small eps it would dominate.)
//   soft-min        in the D layout a lane holds 64 streamed rows of ONE owned row, so the log-sum-exp is lane-local: every lane
//                   keeps a running (max, sum).  Per tile: the 64 exponents replace the accumulators and give the tile's maximum,
//                   the running sum is rescaled once, and 64 v_exp_f32 on (e - max) are added in ascending register order.  The
//                   maximum that is subtracted is replaced by 0 while it is still -inf (first tile, or every row masked), so no
//                   -inf - -inf arises.
//   groups          k_mmd's scheme: the streamed tiles are cut into GROUPS of gt tiles (gt depends on the streamed row count only,
//                   at most 16 tiles); at the end of a group the two half-waves of an owned row are combined by a shuffle and the
//                   fp32 (max, sum) of the group is written to the workspace, then reset.  The longest fp32 addition chain is the
//                   64 gt + 1 <= 1025 additions of a lane.  gridDim.y hands whole groups to workgroups; k_softmin_reduce merges the
//                   groups in group order in double and writes -eps ln 2 (max + log2 sum).  No atomics: the result is bit-identical
//                   for every split count and from run to run.
#include "fd_pairs.h"

namespace {
using namespace fdp;

constexpr int MAX_GROUP_TILES = 16;  // streamed tiles folded in fp32 before the hand-over to double
constexpr int MAX_STEPS = 256;       // iterations of one fd_sinkhorn_potentials call (the schedule is a kernel argument)
constexpr double LOG2E = 1.4426950408889634074, LN2 = 0.69314718055994530942;

struct SmArgs {
    const float* oc;      // (opad, dp) centred owned rows, opad % TQ == 0
    const float* on;      // (opad)
    const float* sc;      // (spad, dp) centred streamed rows, spad % TR == 0
    const float* sn;      // (spad)
    const float* hs;      // (m) s h_j of the streamed rows
    const double* eps;    // the eps of this pass (device)
    int m, opad, dp;      // m: streamed rows that exist
    int gt, groups, groups_per_split, ntiles;
    float* pmax;          // (groups, opad) the groups' maxima
    float* psum;          // (groups, opad) and sums
};

__device__ __forceinline__ float softmin_scale(double eps) { return (float)(LOG2E / eps); }

// hs[j] = f32((pot[j] + eps log w[j]) s), the product in double; w == null: the uniform weight 1 / m, or (plain) no weight term
__global__ __launch_bounds__(256) void k_softmin_prep(const double* __restrict__ pot, const double* __restrict__ w, int plain,
                                                      const double* __restrict__ eps, int m, float* __restrict__ hs) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const double e = *eps;
    double h = pot[j];
    if (w) h += e * log(w[j]);
    else if (!plain) h -= e * log((double)m);
    hs[j] = (float)(h * (double)softmin_scale(e));
}

__global__ __launch_bounds__(NT, 2) void k_softmin(SmArgs g) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5;
    const int q0 = blockIdx.x * TQ;
    const int gbeg = blockIdx.y * g.groups_per_split, gend = min(g.groups, gbeg + g.groups_per_split);
    const int tbeg = gbeg * g.gt, tend = min(g.ntiles, gend * g.gt), nkc = g.dp / KC;
    const int oi = q0 + 32 * wave + (lane & 31);            // this lane's owned row (< opad)
    const float onorm = g.on[oi];
    const size_t dp = (size_t)g.dp;
    const float nsc = -softmin_scale(*g.eps);               // uniform
    FD_GRAM_ACC(acc);
    float mx = -INFINITY, sm = 0.f;                         // the running (max, sum 2^(e - max)) of this lane's 64 rows per tile

    // aux: [0: s h_j, -inf in the padding by index; 1: ||y_j||^2]
    FD_GRAM_TILES_BEGIN(2, 2, g.oc, g.sc, dp, nkc, q0, 0, tbeg, tend,
                        ra0 = (j < g.m) ? g.hs[j] : -INFINITY;
                        ra1 = g.sn[j];)
        const float* ah = aux[tile & 1][0] + 4 * half;
        const float* an = aux[tile & 1][1] + 4 * half;
        float tm = -INFINITY;
        FD_GRAM_DRAIN(t, i) {
            const int c = FD_GRAM_ROW(0, t, i, 0);
            const float d2 = fmaxf(fmaf(-2.f, acc[t][i], onorm + an[c]), 0.f);
            const float e = fmaf(d2, nsc, ah[c]);
            acc[t][i] = e;
            tm = fmaxf(tm, e);
        }
        const float top = fmaxf(mx, tm), sub = (top == -INFINITY) ? 0.f : top;      // sub is finite: no -inf - -inf below
        sm *= __builtin_amdgcn_exp2f(mx - sub);
        mx = top;
        FD_GRAM_DRAIN(t, i) {
            sm += __builtin_amdgcn_exp2f(acc[t][i] - sub);
            acc[t][i] = 0.f;
        }

        if ((tile + 1) % g.gt == 0 || tile + 1 == tend) {
            // end of a group: the upper half-wave holds the other 64 gt streamed rows of the same owned rows
            const float omx = __shfl_down(mx, 32), osm = __shfl_down(sm, 32);
            const float both = fmaxf(mx, omx), bsub = (both == -INFINITY) ? 0.f : both;
            const float s = sm * __builtin_amdgcn_exp2f(mx - bsub) + osm * __builtin_amdgcn_exp2f(omx - bsub);
            if (lane < 32) {
                const size_t o = (size_t)(tile / g.gt) * g.opad + oi;
                g.pmax[o] = both;
                g.psum[o] = s;
            }
            mx = -INFINITY;
            sm = 0.f;
        }
    FD_GRAM_TILES_END
}

// out[i] = -eps ln 2 (M + log2 S) with (M, S) the groups' (max, sum) merged in group order in double; average: the symmetric
// Sinkhorn step out[i] = (out[i] + that) / 2
__global__ __launch_bounds__(256) void k_softmin_reduce(const float* __restrict__ pmax, const float* __restrict__ psum, int groups,
                                                        int opad, int n, const double* __restrict__ eps, int average,
                                                        double* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double M = 0.0, S = 0.0;
    for (int z = 0; z < groups; ++z) {
        const double s = (double)psum[(size_t)z * opad + i];
        if (!(s > 0.0)) continue;                           // a group with nothing in it has max -inf
        const double mz = (double)pmax[(size_t)z * opad + i];
        if (S == 0.0) {
            M = mz;
            S = s;
        } else if (mz > M) {
            S = S * exp2(M - mz) + s;
            M = mz;
        } else {
            S += s * exp2(mz - M);
        }
    }
    const double v = -(*eps) * LN2 * (M + log2(S));
    out[i] = average ? 0.5 * (out[i] + v) : v;
}

// ---------------------------------------------------------------------------------------------- the schedule
struct ShSchedule { double eps[MAX_STEPS]; };

// eps_base = 2 sum ss / (N - 1) over the pooled rows (ssx then, unless null, ssy; strided partials, then a fixed tree: k_mmd_bandwidth's
// base2), 1 when every row is the same; eps_dev[k] = sched[k] (absolute) or sched[k] eps_base
__global__ __launch_bounds__(256) void k_sinkhorn_eps(const double* __restrict__ ssx, int n, const double* __restrict__ ssy, int m,
                                                      ShSchedule sched, int n_steps, int absolute, double* __restrict__ eps_dev,
                                                      double* __restrict__ out_base) {
    __shared__ double red[256];
    const int N = n + (ssy ? m : 0);
    double s = 0.0;
    for (int i = threadIdx.x; i < N; i += 256) s += i < n ? ssx[i] : ssy[i - n];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    const double base = (N > 1 && red[0] > 0.0) ? 2.0 * red[0] / (double)(N - 1) : 1.0;
    if (threadIdx.x == 0) *out_base = base;
    for (int k = threadIdx.x; k < n_steps; k += 256) eps_dev[k] = absolute ? sched.eps[k] : sched.eps[k] * base;
}

// ---------------------------------------------------------------------------------------------- host side
// one direction of the pass: `own` rows against `str` streamed rows
struct SmDir {
    int own, str, opad, spad, ntiles, gt, groups, splits, groups_per_split;
};

// forced > 0 (or FDIFF_SOFTMIN_SPLITS): that many splits; else one when the row blocks fill the device, else about two workgroups
// per CU.  A split is a whole number of groups and the group length depends on the streamed row count alone: the partial (max,
// sum) pairs, hence the results, are those of every split.
SmDir sm_dir(const fd_ctx* ctx, int own, int str, int forced) {
    SmDir p;
    p.own = own; p.str = str;
    p.opad = padded_rows(own);
    p.spad = padded_rows(str);
    p.ntiles = p.spad / TR;
    p.gt = std::max(1, std::min(MAX_GROUP_TILES, p.ntiles / 16));
    p.groups = fd_cdiv(p.ntiles, p.gt);
    const int wgs = p.opad / TQ;
    plan_splits("FDIFF_SOFTMIN_SPLITS", forced > 0 ? forced : (wgs < ctx->num_cu ? fd_cdiv(2 * ctx->num_cu, wgs) : 1), p.groups, &p.splits,
                &p.groups_per_split);
    return p;
}

struct SmPlan {
    bool same;
    int dp;
    SmDir xy, yx;         // owned x / streamed y, and the reverse (the iteration only)
    size_t o_pool, o_part, o_meand, o_mean, o_xc, o_xn, o_xs, o_yc, o_yn, o_ys, o_hx, o_hy, o_pmax, o_psum, o_eps, bytes;
};

SmPlan sm_plan(const fd_ctx* ctx, int n, int m, int d, bool same, bool both_ways, int forced) {
    SmPlan p;
    p.same = same;
    p.dp = padded_features(d);
    p.xy = sm_dir(ctx, n, m, forced);
    p.yx = sm_dir(ctx, m, n, forced);
    const int N = same ? n : n + m;
    Carve ws;
    p.o_pool = ws.take(same ? 0 : (size_t)N * d * sizeof(float));
    p.o_part = ws.take((size_t)mean_chunks(N) * d * sizeof(double));
    p.o_meand = ws.take((size_t)p.dp * sizeof(double));
    p.o_mean = ws.take((size_t)p.dp * sizeof(float));
    p.o_xc = ws.take((size_t)p.xy.opad * p.dp * sizeof(float));
    p.o_xn = ws.take((size_t)p.xy.opad * sizeof(float));
    p.o_xs = ws.take((size_t)p.xy.opad * sizeof(double));
    p.o_yc = ws.take(same ? 0 : (size_t)p.xy.spad * p.dp * sizeof(float));
    p.o_yn = ws.take(same ? 0 : (size_t)p.xy.spad * sizeof(float));
    p.o_ys = ws.take(same ? 0 : (size_t)p.xy.spad * sizeof(double));
    p.o_hx = ws.take((size_t)n * sizeof(float));
    p.o_hy = ws.take((size_t)m * sizeof(float));
    size_t part = (size_t)p.xy.groups * p.xy.opad;
    if (both_ways) part = std::max(part, (size_t)p.yx.groups * p.yx.opad);
    p.o_pmax = ws.take(part * sizeof(float));
    p.o_psum = ws.take(part * sizeof(float));
    p.o_eps = ws.take((size_t)MAX_STEPS * sizeof(double));
    p.bytes = ws.bytes();
    return p;
}

struct SmBuffers {
    float *xc, *xn, *yc, *yn, *hx, *hy, *pmax, *psum;
    double *xs, *ys, *eps;
};

// the mean of the pooled rows (a stacked copy, unless the sets are one), the centred copies, norms and double deviations of both
SmBuffers sm_prepare(const SmPlan& p, char* base, const float* x, int n, const float* y, int m, int d, hipStream_t s) {
    SmBuffers b;
    double* meand = (double*)(base + p.o_meand);
    float* mean = (float*)(base + p.o_mean);
    b.xc = (float*)(base + p.o_xc); b.xn = (float*)(base + p.o_xn); b.xs = (double*)(base + p.o_xs);
    b.yc = p.same ? b.xc : (float*)(base + p.o_yc);
    b.yn = p.same ? b.xn : (float*)(base + p.o_yn);
    b.ys = p.same ? nullptr : (double*)(base + p.o_ys);
    b.hx = (float*)(base + p.o_hx); b.hy = (float*)(base + p.o_hy);
    b.pmax = (float*)(base + p.o_pmax); b.psum = (float*)(base + p.o_psum);
    b.eps = (double*)(base + p.o_eps);
    const float* pool = x;
    if (!p.same) {
        float* z = (float*)(base + p.o_pool);
        (void)hipMemcpyAsync(z, x, (size_t)n * d * sizeof(float), hipMemcpyDeviceToDevice, s);
        (void)hipMemcpyAsync(z + (size_t)n * d, y, (size_t)m * d * sizeof(float), hipMemcpyDeviceToDevice, s);
        pool = z;
    }
    centre_mean(pool, p.same ? n : n + m, d, (double*)(base + p.o_part), meand, mean, s);
    centre_rows(x, n, d, mean, meand, b.xc, b.xn, b.xs, s);
    if (!p.same) centre_rows(y, m, d, mean, meand, b.yc, b.yn, b.ys, s);
    return b;
}

// out (own rows) <- the soft-min over the streamed rows of pot + eps log w (plain: of pot), at the eps of *eps
void sm_pass(const SmPlan& p, const SmDir& dir, const SmBuffers& b, bool own_is_x, const double* pot, const double* w, int plain,
             const double* eps, int average, double* out, hipStream_t s) {
    SmArgs g;
    g.oc = own_is_x ? b.xc : b.yc; g.on = own_is_x ? b.xn : b.yn;
    g.sc = own_is_x ? b.yc : b.xc; g.sn = own_is_x ? b.yn : b.xn;
    float* hs = own_is_x ? b.hy : b.hx;
    g.hs = hs; g.eps = eps;
    g.m = dir.str; g.opad = dir.opad; g.dp = p.dp;
    g.gt = dir.gt; g.groups = dir.groups; g.groups_per_split = dir.groups_per_split; g.ntiles = dir.ntiles;
    g.pmax = b.pmax; g.psum = b.psum;
    hipLaunchKernelGGL(k_softmin_prep, dim3(fd_cdiv(dir.str, 256)), dim3(256), 0, s, pot, w, plain, eps, dir.str, hs);
    hipLaunchKernelGGL(k_softmin, dim3(dir.opad / TQ, dir.splits), dim3(NT), 0, s, g);
    hipLaunchKernelGGL(k_softmin_reduce, dim3(fd_cdiv(dir.own, 256)), dim3(256), 0, s, b.pmax, b.psum, dir.groups, dir.opad, dir.own, eps,
                       average, out);
}

int sm_check_shape(fd_ctx* ctx, const char* who, int n, int m, int d) {
    FD_REQUIRE(ctx, n >= 1 && m >= 1 && d >= 1, "%s: bad shape n=%d m=%d d=%d (all >= 1)", who, n, m, d);
    FD_REQUIRE(ctx, (long long)n * d < (1ll << 31) && (long long)m * d < (1ll << 31) && (long long)n + m < (1ll << 31),
               "%s: too large (n * d, m * d and n + m must stay below 2^31)", who);
    return FD_OK;
}

}  // namespace

extern "C" int fd_softmin_pairs_workspace_bytes(fd_ctx* ctx, int n, int m, int d, int same, int splits, size_t* bytes) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, bytes, "fd_softmin_pairs_workspace_bytes: null pointer");
    if (int rc = sm_check_shape(ctx, "fd_softmin_pairs_workspace_bytes", n, m, d)) return rc;
    FD_REQUIRE(ctx, splits >= 0, "fd_softmin_pairs_workspace_bytes: splits=%d is negative (0: automatic)", splits);
    FD_REQUIRE(ctx, !same || n == m, "fd_softmin_pairs_workspace_bytes: same needs n == m (n=%d m=%d)", n, m);
    *bytes = sm_plan(ctx, n, m, d, same != 0, false, splits).bytes;
    return FD_OK;
}

extern "C" int fd_softmin_pairs(fd_ctx* ctx, const float* x, int n, const float* y, int m, int d, const double* h, double eps, int splits,
                                double* out, void* work, size_t work_bytes, void* stream) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, x && y && h && out && work, "fd_softmin_pairs: null pointer");
    if (int rc = sm_check_shape(ctx, "fd_softmin_pairs", n, m, d)) return rc;
    FD_REQUIRE(ctx, splits >= 0, "fd_softmin_pairs: splits=%d is negative (0: automatic)", splits);
    FD_REQUIRE(ctx, std::isfinite(eps) && eps > 0.0, "fd_softmin_pairs: eps=%g (finite and > 0)", eps);
    const SmPlan p = sm_plan(ctx, n, m, d, x == y && n == m, false, splits);
    FD_REQUIRE(ctx, work_bytes >= p.bytes, "fd_softmin_pairs: workspace of %zu bytes, fd_softmin_pairs_workspace_bytes asks for %zu",
               work_bytes, p.bytes);
    hipStream_t s = (hipStream_t)stream;
    char* base = Carve::align(work);
    const SmBuffers b = sm_prepare(p, base, x, n, y, m, d, s);
    ShSchedule sched;
    for (int k = 0; k < MAX_STEPS; ++k) sched.eps[k] = eps;
    // eps goes to the device as a one-entry absolute schedule: no rows are summed (eps_base, not needed, lands behind it)
    hipLaunchKernelGGL(k_sinkhorn_eps, dim3(1), dim3(256), 0, s, b.xs, 0, (const double*)nullptr, 0, sched, 1, 1, b.eps, b.eps + 1);
    sm_pass(p, p.xy, b, true, h, nullptr, 1, b.eps, 0, out, s);
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}

extern "C" int fd_sinkhorn_potentials_workspace_bytes(fd_ctx* ctx, int n, int m, int d, int symmetric, size_t* bytes) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, bytes, "fd_sinkhorn_potentials_workspace_bytes: null pointer");
    if (int rc = sm_check_shape(ctx, "fd_sinkhorn_potentials_workspace_bytes", n, m, d)) return rc;
    FD_REQUIRE(ctx, !symmetric || n == m, "fd_sinkhorn_potentials_workspace_bytes: symmetric needs n == m (n=%d m=%d)", n, m);
    *bytes = sm_plan(ctx, n, m, d, symmetric != 0, true, 0).bytes;
    return FD_OK;
}

extern "C" int fd_sinkhorn_potentials(fd_ctx* ctx, const float* x, int n, const float* y, int m, int d, int symmetric, const double* a,
                                      const double* b, const double* eps, int n_steps, int absolute, double* out_f, double* out_g,
                                      double* out_eps_base, void* work, size_t work_bytes, void* stream) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, x && y && eps && out_f && out_g && out_eps_base && work, "fd_sinkhorn_potentials: null pointer");
    if (int rc = sm_check_shape(ctx, "fd_sinkhorn_potentials", n, m, d)) return rc;
    FD_REQUIRE(ctx, !symmetric || (x == y && n == m), "fd_sinkhorn_potentials: symmetric needs x == y and n == m (n=%d m=%d)", n, m);
    FD_REQUIRE(ctx, n_steps >= 1 && n_steps <= MAX_STEPS, "fd_sinkhorn_potentials: n_steps=%d outside [1, %d]", n_steps, MAX_STEPS);
    ShSchedule sched;
    for (int k = 0; k < MAX_STEPS; ++k) {
        sched.eps[k] = k < n_steps ? eps[k] : 1.0;
        FD_REQUIRE(ctx, std::isfinite(sched.eps[k]) && sched.eps[k] > 0.0, "fd_sinkhorn_potentials: eps %d is %g (finite and > 0)", k,
                   sched.eps[k]);
    }
    const SmPlan p = sm_plan(ctx, n, m, d, symmetric != 0, true, 0);
    FD_REQUIRE(ctx, work_bytes >= p.bytes,
               "fd_sinkhorn_potentials: workspace of %zu bytes, fd_sinkhorn_potentials_workspace_bytes asks for %zu", work_bytes, p.bytes);
    hipStream_t s = (hipStream_t)stream;
    char* base = Carve::align(work);
    const SmBuffers bf = sm_prepare(p, base, x, n, y, m, d, s);
    hipLaunchKernelGGL(k_sinkhorn_eps, dim3(1), dim3(256), 0, s, bf.xs, n, bf.ys, m, sched, n_steps, absolute ? 1 : 0, bf.eps, out_eps_base);
    if (symmetric) {
        // p <- (p + softmin_X(p)) / 2 from p = 0; f and g are the one potential
        (void)hipMemsetAsync(out_f, 0, (size_t)n * sizeof(double), s);
        for (int k = 0; k < n_steps; ++k) sm_pass(p, p.xy, bf, true, out_f, a, 0, bf.eps + k, 1, out_f, s);
        if (out_g != out_f) (void)hipMemcpyAsync(out_g, out_f, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s);
    } else {
        // f <- softmin_Y(g), g <- softmin_X(f), from g = 0
        (void)hipMemsetAsync(out_g, 0, (size_t)m * sizeof(double), s);
        for (int k = 0; k < n_steps; ++k) {
            sm_pass(p, p.xy, bf, true, out_g, b, 0, bf.eps + k, 0, out_f, s);
            sm_pass(p, p.yx, bf, false, out_f, a, 0, bf.eps + k, 0, out_g, s);
        }
    }
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}
