// fd_mmd.hip -- the quadratic forms of the kernel two-sample test (NOT in the reference; Gretton et al. 2012).
//
//   fd_kernel_quadforms   quad[p] = sum_{i != j} A[i,p] k(z_i, z_j) A[j,p] for every column p of a 0/1 membership matrix A (N, P),
//                         rowsum[i] = sum_{j != i} k(z_i, z_j) and col0[i] = sum_{j != i} k(z_i, z_j) A[j,0], with the Gaussian
//                         mixture k(a, b) = (1/Q) sum_q exp(-||a - b||^2 / (c_q base2)).  The unbiased MMD^2 of every column (the
//                         observed split and its permutations) is host arithmetic on these (utils/two_sample.py).
//
// One fused kernel (k_mmd): the N x N kernel matrix never exists.
//
//   first product   the centring and the tile loop of fd_pairs.h, which k_nn of fd_neighbours.hip uses too: the pooled rows are
//                   centred by their column mean into a padded copy (here also the double mean and deviations, for the
//                   bandwidth), a workgroup owns 128 rows and streams 128-row tiles (16 features at a time) through the LDS;
//                   d2 = max(0, ||a||^2 + ||b||^2 - 2 a.b) on v_mfma_f32_32x32x2_f32 with the STREAMED rows as A (rows of D) and
//                   the OWNED rows as B (columns).  What follows is this file's: the epilogue of that loop.
//   exponentials    Q v_exp_f32 per pair on d2 * (-log2 e / (c_q base2)), summed in ascending q; the diagonal and the padding are
//                   zeroed by index.  Every step is symmetric in (i, j) and independent of the tile, so k is one symmetric matrix.
//   second product  in the C/D layout register r of a lane holds streamed row 8 (r / 4) + (r % 4) + 4 (lane >> 5) of owned row
//                   lane & 31: exactly the A operand of a 32x32x2 MFMA over the two streamed rows {j, j + 4} (row = lane & 31,
//                   k-slot = lane >> 5).  So the kernel tile goes from the accumulator straight into T (32 owned rows x 32 columns
//                   per accumulator) += k * M, where the B operand M[j + 4 (lane >> 5)][lane & 31] is read from the membership
//                   tile in LDS (bytes, converted on the fly; the packed copy keeps the NPT columns of a lane adjacent, so one
//                   LDS read serves all accumulators).  No LDS round trip of k.
//   columns         P + 1 columns are accumulated: column P is all ones (rowsum).  A workgroup holds NPT in {1, 2, 4, 8}
//                   accumulators (32 NPT columns); beyond 256 columns the column chunks are gridDim.z and every chunk recomputes
//                   the distances (ceil((P + 1) / 256) times in all).
//   groups          T is fp32.  The streamed tiles are cut into GROUPS of gt tiles (gt depends on N only, at most 16 tiles = 2048
//                   rows); at the end of a group T is multiplied by the owned rows' memberships, converted to double, reduced over
//                   the 128 owned rows in a fixed order and written to work, then cleared.  The longest fp32 addition chain of a
//                   term is therefore the 128 gt <= 2048 additions inside T.  gridDim.y (col_splits) hands whole groups to
//                   workgroups; since every group's partial is written separately and k_mmd_reduce adds them in group order, the
//                   result does not depend on the split.  No atomics: two runs are bit-identical.
#include "fd_pairs.h"

namespace {
using namespace fdp;

constexpr int MAX_GROUP_TILES = 16;  // streamed tiles summed in fp32 before the hand-over to double
constexpr int MAX_SCALES = 8, MAX_P = 1024;

// ---------------------------------------------------------------------------------------------- bandwidth, packing
struct MmdScales { double c[MAX_SCALES]; };

// base2 = bandwidth2 > 0 ? bandwidth2 : 2 sum_i ss[i] / (N - 1) (strided partials, then a fixed tree); sc[q] = -log2(e) / (c_q base2)
// rounded to f32.  base2 == 0 (every row the same): sc = 0, every kernel value 1.
__global__ __launch_bounds__(256) void k_mmd_bandwidth(const double* __restrict__ ss, int n, double bandwidth2, MmdScales scales, int nq,
                                                       float* __restrict__ sc, double* __restrict__ out_base2) {
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += ss[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double base2 = bandwidth2 > 0.0 ? bandwidth2 : 2.0 * red[0] / (double)(n - 1);
        *out_base2 = base2;
        for (int q = 0; q < MAX_SCALES; ++q)
            sc[q] = (q < nq && base2 > 0.0) ? (float)(-1.4426950408889634074 / (scales.c[q] * base2)) : 0.f;
    }
}

// where column c of the membership matrix sits in a row of mp: inside its chunk of 32 npt columns, the npt columns {l, l + 32, ...}
// that lane l of the second product feeds to its npt accumulators are adjacent bytes (one LDS read per kernel value)
__host__ __device__ inline int mmd_slot(int c, int npt) {
    const int w = 32 * npt, chunk = c / w, in = c - chunk * w;
    return chunk * w + (in & 31) * npt + (in >> 5);
}

// mp (npad, pw) bytes: the membership matrix with column P all ones, zero in the padded rows and columns, columns at mmd_slot
__global__ __launch_bounds__(256) void k_mmd_pack(const uint8_t* __restrict__ member, uint8_t* __restrict__ mp, int n, int P, int pw,
                                                  int npt, size_t total) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const size_t row = t / (size_t)pw;
    const int c = (int)(t - row * (size_t)pw);
    uint8_t v = 0;
    if (row < (size_t)n) v = c < P ? (member[row * (size_t)P + c] != 0 ? 1 : 0) : (c == P ? 1 : 0);
    mp[row * (size_t)pw + mmd_slot(c, npt)] = v;
}

// ---------------------------------------------------------------------------------------------- the fused kernel
struct MmdArgs {
    const float* zc;      // (npad, dp) centred rows, npad % 128 == 0
    const float* zn;      // (npad)
    const uint8_t* mp;    // (npad, pw), columns at mmd_slot
    const float* sc;      // (8) exponent factors
    int n, npad, dp, nq, P, pw;
    int gt, groups, groups_per_split, ntiles;
    double* qpart;        // (groups, row blocks, pw)
    double* rpart;        // (groups, 2, npad): col0, rowsum
};

template <int NPT>
__global__ __launch_bounds__(NT, 2) void k_mmd(MmdArgs g) {
    constexpr int W = 32 * NPT, MS = W + 8;  // MS: rows j and j + 4 of the membership tile fall into different banks
    static_assert(NPT == 1 || NPT == 2 || NPT == 4 || NPT == 8, "one LDS read of NPT bytes per kernel value");
    __shared__ __attribute__((aligned(8))) uint8_t Ms[TR * MS];
    __shared__ double red[4][NPT][32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int q0 = blockIdx.x * TQ, pbase = blockIdx.z * W;
    const int gbeg = blockIdx.y * g.groups_per_split, gend = min(g.groups, gbeg + g.groups_per_split);
    const int tbeg = gbeg * g.gt, tend = min(g.ntiles, gend * g.gt), nkc = g.dp / KC;
    const int oi = q0 + 32 * wave + l31;                    // this lane's owned row (< npad)
    const float onorm = g.zn[oi];
    const size_t dp = (size_t)g.dp, pw = (size_t)g.pw;
    float sc[MAX_SCALES];                                   // uniform: scalar registers
#pragma unroll
    for (int q = 0; q < MAX_SCALES; ++q) sc[q] = g.sc[q];

    FD_GRAM_ACC(acc);
    f32x16 T[NPT];
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt)
#pragma unroll
        for (int i = 0; i < 16; ++i) T[pt][i] = 0.f;

    // aux: ||z_j||^2 of the streamed rows
    FD_GRAM_TILES_BEGIN(1, 1, g.zc, g.zc, dp, nkc, q0, 0, tbeg, tend, ra0 = g.zn[j];)
        // the membership rows of this tile: every earlier reader of Ms is behind the barriers of the loop above
        const int j0 = tile * TR;
        for (int id = tid; id < TR * (W / 8); id += NT) {
            const int row = id / (W / 8), c8 = id - row * (W / 8);
            *reinterpret_cast<uint2*>(Ms + row * MS + 8 * c8) =
                *reinterpret_cast<const uint2*>(g.mp + (size_t)(j0 + row) * pw + pbase + 8 * c8);
        }
        __syncthreads();
        // D layout: register i of accumulator t -> streamed row 32 t + 8 (i / 4) + 4 (lane >> 5) + (i % 4) of the tile, column = this
        // lane's owned row.  As the A operand of the second product that register is (row = owned row, k-slot = lane >> 5) over the
        // streamed rows {rl, rl + 4}; the B operand of k-slot lane >> 5 is the membership row of the same rl.
        // Everything that depends on the lane is in three bases, so that every (t, i) below adds a compile-time constant c to them.
        const int jb = j0 + 4 * half, dself = oi - jb, dend = g.n - jb;      // c == dself: the diagonal; c >= dend: the padding
        const float* an = aux[tile & 1][0] + 4 * half;
        const uint8_t* mlane = Ms + 4 * half * MS + l31 * NPT;
        FD_GRAM_DRAIN(t, i) {
                const int c = FD_GRAM_ROW(0, t, i, 0);
                const float d2 = fmaxf(fmaf(-2.f, acc[t][i], onorm + an[c]), 0.f);
                acc[t][i] = 0.f;
                float kv = __builtin_amdgcn_exp2f(d2 * sc[0]);
#pragma unroll
                for (int q = 1; q < MAX_SCALES; ++q)
                    if (q < g.nq) kv += __builtin_amdgcn_exp2f(d2 * sc[q]);
                kv = (c == dself || c >= dend) ? 0.f : kv;       // the diagonal and the padding, by index
                // the NPT membership bytes of this lane's streamed row: columns l31, l31 + 32, ... of the chunk
                unsigned lo = 0, hi = 0;
                if constexpr (NPT == 8) {
                    const uint2 v = *reinterpret_cast<const uint2*>(mlane + c * MS);
                    lo = v.x; hi = v.y;
                } else if constexpr (NPT == 4) {
                    lo = *reinterpret_cast<const unsigned*>(mlane + c * MS);
                } else if constexpr (NPT == 2) {
                    lo = *reinterpret_cast<const unsigned short*>(mlane + c * MS);
                } else {
                    lo = mlane[c * MS];
                }
#pragma unroll
                for (int pt = 0; pt < NPT; ++pt) {
                    const float b = (float)(((pt < 4 ? lo : hi) >> (8 * (pt & 3))) & 0xffu);
                    T[pt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kv, b, T[pt], 0, 0, 0);
                }
            }

        if ((tile + 1) % g.gt == 0 || tile + 1 == tend) {
            // end of a group: T (owned row 8 (r / 4) + 4 (lane >> 5) + (r % 4) of this wave, column pbase + 32 pt + (lane & 31)) goes to
            // double.  quad: times the owned row's membership, rows in ascending r, the upper half-wave onto the lower, waves in order.
            const int grp = tile / g.gt;
#pragma unroll
            for (int pt = 0; pt < NPT; ++pt) {
                const int col = pbase + 32 * pt + l31, slot = pbase + l31 * NPT + pt;
                double s = 0.0;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = FD_GRAM_ROW(q0 + 32 * wave, 0, r, half);
                    const float v = T[pt][r];
                    s += g.mp[(size_t)row * pw + slot] ? (double)v : 0.0;
                    if (row < g.n) {
                        if (col == 0) g.rpart[((size_t)grp * 2 + 0) * g.npad + row] = (double)v;
                        if (col == g.P) g.rpart[((size_t)grp * 2 + 1) * g.npad + row] = (double)v;
                    }
                    T[pt][r] = 0.f;
                }
                s += __shfl_down(s, 32);
                if (lane < 32) red[wave][pt][lane] = s;
            }
            __syncthreads();
            if (tid < W) {
                const int pt = tid >> 5, l = tid & 31;
                const double s = ((red[0][pt][l] + red[1][pt][l]) + red[2][pt][l]) + red[3][pt][l];
                g.qpart[((size_t)grp * gridDim.x + blockIdx.x) * pw + pbase + tid] = s;
            }
            // red is rewritten at the next group's end, behind the barriers of at least one more tile
        }
    FD_GRAM_TILES_END
}

// quad[p] = inv_q * sum over (group, row block) in ascending order; rowsum / col0 [i] = inv_q * sum over groups
__global__ __launch_bounds__(256) void k_mmd_reduce(const double* __restrict__ qpart, const double* __restrict__ rpart, int groups, int rb,
                                                    int pw, int npad, int n, int P, int pblocks, double inv_q, double* __restrict__ quad,
                                                    double* __restrict__ rowsum, double* __restrict__ col0) {
    if ((int)blockIdx.x < pblocks) {
        const int p = blockIdx.x * 256 + threadIdx.x;
        if (p >= P) return;
        const size_t cnt = (size_t)groups * rb;
        double s = 0.0;
#pragma unroll 8
        for (size_t z = 0; z < cnt; ++z) s += qpart[z * (size_t)pw + p];
        quad[p] = s * inv_q;
    } else {
        const int i = (blockIdx.x - pblocks) * 256 + threadIdx.x;
        if (i >= n) return;
        double a = 0.0, b = 0.0;
        for (int z = 0; z < groups; ++z) {
            a += rpart[((size_t)z * 2 + 0) * npad + i];
            b += rpart[((size_t)z * 2 + 1) * npad + i];
        }
        rowsum[i] = b * inv_q;
        if (col0) col0[i] = a * inv_q;
    }
}

// ---------------------------------------------------------------------------------------------- host side
struct MmdPlan {
    int dp, npad, ntiles, gt, groups, splits, groups_per_split, npt, pch, pw;
    size_t o_part, o_meand, o_mean, o_zc, o_zn, o_ss, o_sc, o_mp, o_qpart, o_rpart, bytes;
};

// col_splits = 0: one split when the row blocks (times the column chunks) fill the device, else about two workgroups per CU.  A split
// is a whole number of groups, and the group length depends on N alone: the partial sums, hence the results, are those of every split.
MmdPlan mmd_plan(const fd_ctx* ctx, int N, int d, int P, int col_splits) {
    MmdPlan p;
    p.dp = padded_features(d);
    p.npad = padded_rows(N);
    p.ntiles = p.npad / TR;
    p.gt = std::max(1, std::min(MAX_GROUP_TILES, p.ntiles / 16));
    p.groups = fd_cdiv(p.ntiles, p.gt);
    const int pc = P + 1;
    p.npt = pc <= 32 ? 1 : pc <= 64 ? 2 : pc <= 128 ? 4 : 8;
    p.pch = fd_cdiv(pc, 32 * p.npt);
    p.pw = p.pch * 32 * p.npt;
    const int wgs = p.ntiles * p.pch;
    int s = col_splits > 0 ? col_splits : (wgs < ctx->num_cu ? fd_cdiv(2 * ctx->num_cu, wgs) : 1);
    s = std::min(s, p.groups);
    p.groups_per_split = fd_cdiv(p.groups, s);
    p.splits = fd_cdiv(p.groups, p.groups_per_split);
    Carve ws;
    p.o_part = ws.take((size_t)mean_chunks(N) * d * sizeof(double));
    p.o_meand = ws.take((size_t)p.dp * sizeof(double));
    p.o_mean = ws.take((size_t)p.dp * sizeof(float));
    p.o_zc = ws.take((size_t)p.npad * p.dp * sizeof(float));
    p.o_zn = ws.take((size_t)p.npad * sizeof(float));
    p.o_ss = ws.take((size_t)p.npad * sizeof(double));
    p.o_sc = ws.take(MAX_SCALES * sizeof(float));
    p.o_mp = ws.take((size_t)p.npad * p.pw);
    p.o_qpart = ws.take((size_t)p.groups * p.ntiles * p.pw * sizeof(double));
    p.o_rpart = ws.take((size_t)p.groups * 2 * p.npad * sizeof(double));
    p.bytes = ws.bytes();
    return p;
}

int mmd_check_shape(fd_ctx* ctx, const char* who, int N, int d, int P, int col_splits) {
    FD_REQUIRE(ctx, N >= 2 && d > 0, "%s: bad shape N=%d d=%d (N >= 2, d >= 1)", who, N, d);
    FD_REQUIRE(ctx, P >= 1 && P <= MAX_P, "%s: P=%d outside [1, %d]", who, P, MAX_P);
    FD_REQUIRE(ctx, col_splits >= 0, "%s: col_splits=%d is negative (0: automatic)", who, col_splits);
    FD_REQUIRE(ctx, (long long)N * d < (1ll << 31) && (long long)N * P < (1ll << 31), "%s: too large (N * d and N * P must stay below 2^31)",
               who);
    return FD_OK;
}

}  // namespace

extern "C" int fd_kernel_quadforms_workspace_bytes(fd_ctx* ctx, int N, int d, int P, int col_splits, size_t* bytes) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, bytes, "fd_kernel_quadforms_workspace_bytes: null pointer");
    if (int rc = mmd_check_shape(ctx, "fd_kernel_quadforms_workspace_bytes", N, d, P, col_splits)) return rc;
    *bytes = mmd_plan(ctx, N, d, P, col_splits).bytes;
    return FD_OK;
}

extern "C" int fd_kernel_quadforms(fd_ctx* ctx, const float* z, int N, int d, const double* scales, int n_scales, double bandwidth2,
                                   const uint8_t* member, int P, int col_splits, double* out_quad, double* out_rowsum, double* out_col0,
                                   double* out_base2, void* work, size_t work_bytes, void* stream) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, z && scales && member && out_quad && out_rowsum && out_base2 && work, "fd_kernel_quadforms: null pointer");
    if (int rc = mmd_check_shape(ctx, "fd_kernel_quadforms", N, d, P, col_splits)) return rc;
    FD_REQUIRE(ctx, n_scales >= 1 && n_scales <= MAX_SCALES, "fd_kernel_quadforms: n_scales=%d outside [1, %d]", n_scales, MAX_SCALES);
    MmdScales sc;
    for (int q = 0; q < MAX_SCALES; ++q) {
        sc.c[q] = q < n_scales ? scales[q] : 1.0;
        FD_REQUIRE(ctx, std::isfinite(sc.c[q]) && sc.c[q] > 0.0, "fd_kernel_quadforms: scale %d is %g (finite and > 0)", q, sc.c[q]);
    }
    FD_REQUIRE(ctx, std::isfinite(bandwidth2), "fd_kernel_quadforms: bandwidth2 is not finite");
    const MmdPlan p = mmd_plan(ctx, N, d, P, col_splits);
    FD_REQUIRE(ctx, work_bytes >= p.bytes, "fd_kernel_quadforms: workspace of %zu bytes, fd_kernel_quadforms_workspace_bytes asks for %zu",
               work_bytes, p.bytes);
    hipStream_t s = (hipStream_t)stream;
    char* base = Carve::align(work);
    double* meand = (double*)(base + p.o_meand);
    float* mean = (float*)(base + p.o_mean);
    float* zc = (float*)(base + p.o_zc);
    float* zn = (float*)(base + p.o_zn);
    double* ss = (double*)(base + p.o_ss);
    float* scf = (float*)(base + p.o_sc);
    uint8_t* mp = (uint8_t*)(base + p.o_mp);
    centre_mean(z, N, d, (double*)(base + p.o_part), meand, mean, s);
    centre_rows(z, N, d, mean, meand, zc, zn, ss, s);       // ss: ||z_i - mean||^2 in double, the bandwidth's closed form
    hipLaunchKernelGGL(k_mmd_bandwidth, dim3(1), dim3(256), 0, s, ss, N, bandwidth2, sc, n_scales, scf, out_base2);
    const size_t mp_total = (size_t)p.npad * p.pw;
    hipLaunchKernelGGL(k_mmd_pack, dim3((unsigned)((mp_total + 255) / 256)), dim3(256), 0, s, member, mp, N, P, p.pw, p.npt, mp_total);

    MmdArgs g;
    g.zc = zc; g.zn = zn; g.mp = mp; g.sc = scf;
    g.n = N; g.npad = p.npad; g.dp = p.dp; g.nq = n_scales; g.P = P; g.pw = p.pw;
    g.gt = p.gt; g.groups = p.groups; g.groups_per_split = p.groups_per_split; g.ntiles = p.ntiles;
    g.qpart = (double*)(base + p.o_qpart);
    g.rpart = (double*)(base + p.o_rpart);
    const dim3 grid(p.ntiles, p.splits, p.pch);
    if (p.npt == 1) hipLaunchKernelGGL(k_mmd<1>, grid, dim3(NT), 0, s, g);
    else if (p.npt == 2) hipLaunchKernelGGL(k_mmd<2>, grid, dim3(NT), 0, s, g);
    else if (p.npt == 4) hipLaunchKernelGGL(k_mmd<4>, grid, dim3(NT), 0, s, g);
    else hipLaunchKernelGGL(k_mmd<8>, grid, dim3(NT), 0, s, g);
    const int pblocks = fd_cdiv(P, 256);
    hipLaunchKernelGGL(k_mmd_reduce, dim3(pblocks + fd_cdiv(N, 256)), dim3(256), 0, s, g.qpart, g.rpart, p.groups, p.ntiles, p.pw, p.npad,
                       N, P, pblocks, 1.0 / (double)n_scales, out_quad, out_rowsum, out_col0);
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}
