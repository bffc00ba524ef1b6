// fd_dependence.hip -- the dependence structure INSIDE a series (NOT in the reference; the autocorrelation difference of TSGBench,
// the correlational score of Ni et al. / Diffusion-TS): per series and channel the first four moments, the
// normalised autocorrelation at lags 1..L and the normalised cross-correlation of every ordered channel pair at lags 0..Lx, plus
// the mean of every feature over the set.
//
//   fd_series_dependence    one fused kernel (k_dependence) and a fixed-order, two-level reduction of the chunk sums
//
// A GROUP of 1, 4 or 16 waves owns one series at a time: it is read from HBM once (coalesced dword loads: a series of 187 floats
// does not start on a 16-byte boundary), transposed into the LDS as buf[c][t] with an ODD row stride Ts >= T + 24 whose tail stays
// zero, and everything else comes out of the LDS.
//
//   centring        P = the largest power of two <= 64 / C lanes share a channel (P depends on C alone): each sums its strided
//                   entries in DOUBLE, a butterfly adds the P partial sums, mu = sum / T.  T equal floats v give k v exactly at
//                   every partial sum (k <= 1024: 34 bits), so mu = v and e = 0 exactly.  e = f32(x - mu), the difference taken
//                   in double BEFORE any product, replaces x in the LDS; S2, S3, S4 = sum e^2, e^3, e^4 in double on the way.
//   lag products    a UNIT is (c, d, block of LB lags); a thread owns units u = gtid, gtid + gsize, ...  It walks t in steps of U
//                   (4; 8 and 16 for LB = 2 and 1) with e[t..t+U-1, c] and the window e[t+l0..t+l0+U+LB-2, d] in registers: U LB
//                   double fmas on 2 U + LB - 1 LDS reads.  Every lag's sum runs over t = 0, 1, 2, ... in that order whatever LB is (the zero tail supplies the
//                   terms past T - 1 - l), so a value depends on (series, T, c, d, l) alone: not on LB, the group size, the grid
//                   or the outputs asked for.  Lanes of a wave differ in d (distinct rows: odd stride, no bank conflict) and
//                   mostly share c (broadcast); for C = 1 they differ in the lag (consecutive addresses).
//   normalisation   value = f32(sum / sqrt(S2c S2d)); 0 when either channel is constant.  The diagonal units (c, c) serve acf and
//                   ccf at once: ccf[l, c, c] IS acf[l - 1, c].
//   set means       series are cut into chunks of DEP_CHUNK = 32; a group owns whole chunks and every feature has ONE owner thread
//                   whose double accumulator lives in an LDS cell of its own; at the end of a chunk the cells go to part[chunk][f];
//                   k_dep_super_sums adds the chunks of every 64 in order and k_dep_set_mean those sums in order.  No atomics: bit-identical for every grid (FDIFF_DEP_SPLITS)
//                   and from run to run.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "fd_pairs.h"

namespace {
using fdp::Carve;

constexpr int DEP_CHUNK = 32;        // series per partial sum of the set means
constexpr int DEP_SUPER = 64;        // chunks per second-level partial sum
constexpr int DEP_MAX_T = 1024, DEP_MAX_C = 64;
constexpr int DEP_PREFETCH = 4;      // floats of the next series a thread holds in registers while it works on this one
constexpr size_t DEP_MAX_LDS = 160 * 1024;

struct DepArgs {
    const float* x;
    int n, T, C, L, Lx;
    int Ts;                 // LDS row stride (floats), odd, >= T + 24
    int P;                  // lanes per channel in the centring
    int gsize;              // threads of a group
    int nlb_x;              // lag blocks of an off-diagonal pair (lags 0..Lx)
    int n_xunits, n_units;  // C C nlb_x units of every ordered pair, then the diagonal's further blocks up to lag max(L, Lx)
    int rounds;             // units per thread
    int chunks, chunks_per_group;
    int prefetch;           // the next series fits the prefetch registers
    int group_bytes;        // LDS of one group
    int F;
    float* out_mom;         // (n, C, 4) or null
    float* out_acf;         // (n, L, C) or null
    float* out_ccf;         // (n, Lx + 1, C, C) or null
    double* part;           // (chunks, F) or null
};

// time steps per register window: a short lag block takes more steps, so that as many LDS reads are in flight (the loop is bound by
// their latency when few waves share a CU); the values do not depend on it
constexpr int dep_steps(int LB) { return LB == 1 ? 16 : LB == 2 ? 8 : 4; }

__device__ __forceinline__ double dep_butterfly(double v, int P) {
    for (int o = P >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <int LB>
__global__ __launch_bounds__(1024) void k_dependence(DepArgs g) {
    constexpr int U = dep_steps(LB);
    extern __shared__ double dep_smem[];
    const int T = g.T, C = g.C, L = g.L, Lx = g.Lx, Ts = g.Ts, gsz = g.gsize, TC = T * C;
    const int tid = threadIdx.x, grp = tid / gsz, gtid = tid - grp * gsz, gpb = blockDim.x / gsz;
    char* base = (char*)dep_smem + (size_t)grp * g.group_bytes;
    double* acc = (double*)base;                            // (LB, n_units): cell (j, u) belongs to the owner of unit u
    double* macc = acc + (size_t)LB * g.n_units;       // (4, C) moment sums, owned by lane p == 0 of the channel
    double* S2 = macc + 4 * C;                              // (C) sum e^2 of the current series
    float* buf = (float*)(S2 + C);                          // (C, Ts)

    for (int i = gtid; i < LB * g.n_units + 4 * C; i += gsz) acc[i] = 0.0;
    for (int i = gtid; i < C * Ts; i += gsz) buf[i] = 0.f;
    __syncthreads();

    const int chunk0 = (blockIdx.x * gpb + grp) * g.chunks_per_group;
    const int nslots = g.chunks_per_group * DEP_CHUNK;      // the same for every group: the barriers below are uniform
    const int P = g.P, p = gtid & (P - 1), CC = C * C;
    const size_t acf_off = (size_t)4 * C, ccf_off = acf_off + (size_t)L * C;

    float pre[DEP_PREFETCH];
    bool have_pre = false;
    for (int slot = 0; slot < nslots; ++slot) {
        const int chunk = chunk0 + slot / DEP_CHUNK;
        const long long s = (long long)chunk * DEP_CHUNK + slot % DEP_CHUNK;
        const bool live = chunk < g.chunks && s < g.n;
        if (live) {
            const float* xs = g.x + (size_t)s * TC;
            if (have_pre) {
#pragma unroll
                for (int k = 0; k < DEP_PREFETCH; ++k) {
                    const int i = gtid + k * gsz;
                    if (i < TC) {
                        const int t = i / C;
                        buf[(i - t * C) * Ts + t] = pre[k];
                    }
                }
            } else {
                for (int i = gtid; i < TC; i += gsz) {
                    const int t = i / C;
                    buf[(i - t * C) * Ts + t] = xs[i];
                }
            }
        }
        __syncthreads();

        // ---- centring and moments: lane p of the P lanes of channel c takes t = p, p + P, ...
        if (live) {
            for (int c = gtid / P; c < C; c += gsz / P) {
                float* row = buf + c * Ts;
                double sum = 0.0;
                for (int t = p; t < T; t += P) sum += (double)row[t];
                const double mu = dep_butterfly(sum, P) / (double)T;
                double s2 = 0.0, s3 = 0.0, s4 = 0.0;
                for (int t = p; t < T; t += P) {
                    const float e = (float)((double)row[t] - mu);
                    row[t] = e;
                    const double ed = (double)e, e2 = ed * ed;
                    s2 += e2;
                    s3 += e2 * ed;
                    s4 += e2 * e2;
                }
                s2 = dep_butterfly(s2, P);
                s3 = dep_butterfly(s3, P);
                s4 = dep_butterfly(s4, P);
                if (p == 0) {
                    S2[c] = s2;
                    const double m2 = s2 / (double)T;
                    float mom[4] = {(float)mu, (float)sqrt(m2), 0.f, 0.f};
                    if (s2 > 0.0) {
                        mom[2] = (float)((s3 / (double)T) / (m2 * sqrt(m2)));
                        mom[3] = (float)((s4 / (double)T) / (m2 * m2) - 3.0);
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if (g.out_mom) g.out_mom[((size_t)s * C + c) * 4 + k] = mom[k];
                        macc[k * C + c] += (double)mom[k];
                    }
                }
            }
        }
        __syncthreads();

        // ---- the next series travels while this one is multiplied
        have_pre = false;
        if (g.prefetch && slot + 1 < nslots) {
            const int nchunk = chunk0 + (slot + 1) / DEP_CHUNK;
            const long long ns = (long long)nchunk * DEP_CHUNK + (slot + 1) % DEP_CHUNK;
            if (nchunk < g.chunks && ns < g.n) {
                const float* xs = g.x + (size_t)ns * TC;
#pragma unroll
                for (int k = 0; k < DEP_PREFETCH; ++k) {
                    const int i = gtid + k * gsz;
                    pre[k] = i < TC ? xs[i] : 0.f;
                }
                have_pre = true;
            }
        }

        // ---- lag products
        if (live) {
            int u = gtid;
            for (int k = 0; k < g.rounds && u < g.n_units; ++k, u += gsz) {
                int c, d, lb;
                if (u < g.n_xunits) {
                    lb = u / CC;
                    const int r = u - lb * CC;
                    c = r / C;
                    d = r - c * C;
                } else {
                    const int v = u - g.n_xunits;
                    lb = g.nlb_x + v / C;
                    c = d = v - (v / C) * C;
                }
                const int lag0 = lb * LB;
                const float* a = buf + c * Ts;
                const float* w = buf + d * Ts + lag0;
                double dot[LB];
#pragma unroll
                for (int j = 0; j < LB; ++j) dot[j] = 0.0;
                for (int t0 = 0; t0 < T - lag0; t0 += U) {
                    float av[U], wv[U + LB - 1];
#pragma unroll
                    for (int i = 0; i < U; ++i) av[i] = a[t0 + i];
#pragma unroll
                    for (int i = 0; i < U + LB - 1; ++i) wv[i] = w[t0 + i];
#pragma unroll
                    for (int i = 0; i < U; ++i)
#pragma unroll
                        for (int j = 0; j < LB; ++j) dot[j] = fma((double)av[i], (double)wv[i + j], dot[j]);
                }
                const double den = S2[c] * S2[d];
                const double inv = den > 0.0 ? 1.0 / sqrt(den) : 0.0;
#pragma unroll
                for (int j = 0; j < LB; ++j) {
                    const int l = lag0 + j;
                    const float v = (float)(dot[j] * inv);
                    bool used = false;
                    if (l <= Lx) {
                        if (g.out_ccf) g.out_ccf[(((size_t)s * (Lx + 1) + l) * C + c) * C + d] = v;
                        used = true;
                    }
                    if (c == d && l >= 1 && l <= L) {
                        if (g.out_acf) g.out_acf[((size_t)s * L + (l - 1)) * C + c] = v;
                        used = true;
                    }
                    if (used) acc[(size_t)j * g.n_units + u] += (double)v;
                }
            }
        }

        // ---- end of a chunk: every owner hands its sums over and starts again from zero
        if (slot % DEP_CHUNK == DEP_CHUNK - 1 && chunk < g.chunks) {
            double* part = g.part ? g.part + (size_t)chunk * g.F : nullptr;
            if (p == 0) {
                for (int c = gtid / P; c < C; c += gsz / P) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if (part) part[c * 4 + k] = macc[k * C + c];
                        macc[k * C + c] = 0.0;
                    }
                }
            }
            int u = gtid;
            for (int k = 0; k < g.rounds && u < g.n_units; ++k, u += gsz) {
                int c, d, lb;
                if (u < g.n_xunits) {
                    lb = u / CC;
                    const int r = u - lb * CC;
                    c = r / C;
                    d = r - c * C;
                } else {
                    const int v = u - g.n_xunits;
                    lb = g.nlb_x + v / C;
                    c = d = v - (v / C) * C;
                }
                for (int j = 0; j < LB; ++j) {
                    const int l = lb * LB + j;
                    double* cell = acc + (size_t)j * g.n_units + u;
                    if (part) {
                        if (l <= Lx) part[ccf_off + ((size_t)l * C + c) * C + d] = *cell;
                        if (c == d && l >= 1 && l <= L) part[acf_off + (size_t)(l - 1) * C + c] = *cell;
                    }
                    *cell = 0.0;
                }
            }
        }
        __syncthreads();
    }
}

// The chunk sums are added in two fixed levels (a thread that adds thousands of them one load at a time waits for every load):
// level 1 adds the chunks of a SUPER-chunk of DEP_SUPER = 64 chunks in chunk order, level 2 the super-chunks in order and divides
// by n.  The loads of 16 terms are issued together, the additions stay in order.  The grouping depends on n alone.
__device__ __forceinline__ double dep_sum_in_order(const double* __restrict__ p, int count, size_t stride) {
    double s = 0.0;
    for (int z0 = 0; z0 < count; z0 += 16) {
        double v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = z0 + j < count ? p[(size_t)(z0 + j) * stride] : 0.0;
#pragma unroll
        for (int j = 0; j < 16; ++j) s += v[j];
    }
    return s;
}

__global__ __launch_bounds__(256) void k_dep_super_sums(const double* __restrict__ part, int chunks, int F, double* __restrict__ sup) {
    const int f = blockIdx.y * 256 + threadIdx.x, z0 = blockIdx.x * DEP_SUPER;
    if (f >= F) return;
    sup[(size_t)blockIdx.x * F + f] = dep_sum_in_order(part + (size_t)z0 * F + f, min(DEP_SUPER, chunks - z0), (size_t)F);
}

__global__ __launch_bounds__(256) void k_dep_set_mean(const double* __restrict__ sup, int supers, int F, int n, double* __restrict__ out) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    out[f] = dep_sum_in_order(sup + f, supers, (size_t)F) / (double)n;
}

// ---------------------------------------------------------------------------------------------- host side
struct DepPlan {
    DepArgs a;
    int LB, gpb, grid;
    size_t lds_bytes, o_part, o_sup, bytes;
    int supers;
};

int dep_blocks(int lags, int LB) { return lags > 0 ? fd_cdiv(lags, LB) : 0; }

// Everything but the grid is a function of (T, C, L, Lx); nothing a value depends on is a function of anything but (T, C).
int dep_plan(fd_ctx* ctx, const char* who, int n, int T, int C, int L, int Lx, DepPlan* out) {
    FD_REQUIRE(ctx, n >= 1 && T >= 1 && C >= 1, "%s: bad shape n=%d T=%d C=%d (all >= 1)", who, n, T, C);
    FD_REQUIRE(ctx, T <= DEP_MAX_T && C <= DEP_MAX_C, "%s: T=%d C=%d: at most T=%d and C=%d", who, T, C, DEP_MAX_T, DEP_MAX_C);
    FD_REQUIRE(ctx, L >= 0 && L <= T - 1, "%s: acf_lags=%d outside [0, T - 1 = %d]", who, L, T - 1);
    FD_REQUIRE(ctx, Lx >= -1 && Lx <= T - 1, "%s: ccf_lags=%d outside [-1, T - 1 = %d] (-1: no ccf)", who, Lx, T - 1);
    const long long F = 4ll * C + (long long)L * C + (long long)(Lx + 1) * C * C;
    FD_REQUIRE(ctx, (long long)n * F < (1ll << 31) && (long long)n * T * C < (1ll << 31),
               "%s: too large (n * F = %lld and n * T * C = %lld must stay below 2^31)", who, (long long)n * F, (long long)n * T * C);
    DepPlan p;
    DepArgs& a = p.a;
    a.n = n; a.T = T; a.C = C; a.L = L; a.Lx = Lx; a.F = (int)F;
    a.Ts = (T + 24) | 1;                                             // a window reads up to index T + U + LB - 3 <= T + 14
    a.P = 1;
    while (a.P * 2 * C <= 64) a.P *= 2;
    const int nx = Lx + 1, nd = std::max(L, Lx) + 1;                 // lags of an off-diagonal pair / of the diagonal, lag 0 included
    const long long slots = (long long)C * C * nx + (long long)C * (nd - nx);
    const int G = slots <= 512 ? 1 : slots <= 8192 ? 4 : 16;
    a.gsize = 64 * G;
    // the lag block: cheapest per useful lag (LDS reads against fmas, both per 4 time steps) among those that give every thread a unit
    static const int cand[5] = {9, 8, 4, 2, 1};
    p.LB = 1;
    double best = 0.0;
    for (int LB : cand) {
        const long long units = (long long)C * C * dep_blocks(nx, LB) + (long long)C * (dep_blocks(nd, LB) - dep_blocks(nx, LB));
        if (units < a.gsize && LB != 1) continue;
        const int U = dep_steps(LB);
        const double cost = (double)fd_cdiv(units, a.gsize) * std::max(2 * (2 * U + LB - 1), U * LB) / U;
        if (best == 0.0 || cost < best) { best = cost; p.LB = LB; }
    }
    a.nlb_x = dep_blocks(nx, p.LB);
    a.n_xunits = C * C * a.nlb_x;
    a.n_units = a.n_xunits + C * (dep_blocks(nd, p.LB) - a.nlb_x);
    a.rounds = fd_cdiv(a.n_units, a.gsize);
    a.prefetch = T * C <= DEP_PREFETCH * a.gsize ? 1 : 0;
    const size_t gb = 8 * ((size_t)p.LB * a.n_units + 5 * (size_t)C) + 4 * (size_t)C * a.Ts;
    a.group_bytes = (int)((gb + 7) & ~(size_t)7);
    FD_REQUIRE(ctx, (size_t)a.group_bytes <= DEP_MAX_LDS,
               "%s: T=%d C=%d acf_lags=%d ccf_lags=%d needs %d bytes of LDS per series (the series and one double per feature), at "
               "most %zu: ask for fewer cross lags", who, T, C, L, Lx, a.group_bytes, DEP_MAX_LDS);
    p.gpb = G == 1 ? 4 : 1;
    while (p.gpb > 1 && (size_t)p.gpb * a.group_bytes > DEP_MAX_LDS) p.gpb /= 2;
    p.lds_bytes = (size_t)p.gpb * a.group_bytes;
    a.chunks = fd_cdiv(n, DEP_CHUNK);
    // the grid: FDIFF_DEP_SPLITS workgroups (tests), else what the device holds at once (16 waves and 160 KiB of LDS per CU)
    const int block_waves = p.gpb * G;
    const int per_cu = std::max(1, std::min(16 / block_waves, (int)(DEP_MAX_LDS / p.lds_bytes)));
    const char* e = getenv("FDIFF_DEP_SPLITS");
    const int forced = e ? atoi(e) : 0;
    const int most = fd_cdiv(a.chunks, p.gpb);
    const int want = std::max(1, std::min(most, forced > 0 ? forced : ctx->num_cu * per_cu));
    a.chunks_per_group = fd_cdiv(a.chunks, want * p.gpb);
    p.grid = fd_cdiv(a.chunks, a.chunks_per_group * p.gpb);
    p.supers = fd_cdiv(a.chunks, DEP_SUPER);
    Carve ws;
    p.o_part = ws.take((size_t)a.chunks * a.F * sizeof(double));
    p.o_sup = ws.take((size_t)p.supers * a.F * sizeof(double));
    p.bytes = ws.bytes();
    *out = p;
    return FD_OK;
}

template <int LB>
int dep_launch(fd_ctx* ctx, const DepPlan& p, hipStream_t s) {
    static unsigned long long attr_set = 0;
    if (p.lds_bytes > 48 * 1024 && fd_first_on_device(attr_set, ctx->device))
        FD_HIP(ctx, hipFuncSetAttribute((const void*)k_dependence<LB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)DEP_MAX_LDS));
    hipLaunchKernelGGL(k_dependence<LB>, dim3(p.grid), dim3(p.gpb * p.a.gsize), p.lds_bytes, s, p.a);
    return FD_OK;
}

}  // namespace

extern "C" int fd_series_dependence_workspace_bytes(fd_ctx* ctx, int n, int T, int C, int acf_lags, int ccf_lags, size_t* bytes) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, bytes, "fd_series_dependence_workspace_bytes: null pointer");
    DepPlan p;
    if (int rc = dep_plan(ctx, "fd_series_dependence_workspace_bytes", n, T, C, acf_lags, ccf_lags, &p)) return rc;
    *bytes = p.bytes;
    return FD_OK;
}

extern "C" int fd_series_dependence(fd_ctx* ctx, const float* x, int n, int T, int C, int acf_lags, int ccf_lags, float* out_moments,
                                    float* out_acf, float* out_ccf, double* out_set_mean, void* work, size_t work_bytes, void* stream) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, x, "fd_series_dependence: null x");
    DepPlan p;
    if (int rc = dep_plan(ctx, "fd_series_dependence", n, T, C, acf_lags, ccf_lags, &p)) return rc;
    FD_REQUIRE(ctx, out_moments || out_acf || out_ccf || out_set_mean, "fd_series_dependence: every output is null");
    FD_REQUIRE(ctx, !out_acf || acf_lags >= 1, "fd_series_dependence: out_acf with acf_lags=0");
    FD_REQUIRE(ctx, !out_ccf || ccf_lags >= 0, "fd_series_dependence: out_ccf with ccf_lags=-1 (no ccf)");
    FD_REQUIRE(ctx, !out_set_mean || (work && work_bytes >= p.bytes),
               "fd_series_dependence: workspace of %zu bytes, fd_series_dependence_workspace_bytes asks for %zu", work ? work_bytes : 0,
               p.bytes);
    hipStream_t s = (hipStream_t)stream;
    p.a.x = x;
    p.a.out_mom = out_moments;
    p.a.out_acf = out_acf;
    p.a.out_ccf = out_ccf;
    char* base = out_set_mean ? Carve::align(work) : nullptr;
    p.a.part = out_set_mean ? (double*)(base + p.o_part) : nullptr;
    int rc = FD_OK;
    switch (p.LB) {
        case 9: rc = dep_launch<9>(ctx, p, s); break;
        case 8: rc = dep_launch<8>(ctx, p, s); break;
        case 4: rc = dep_launch<4>(ctx, p, s); break;
        case 2: rc = dep_launch<2>(ctx, p, s); break;
        default: rc = dep_launch<1>(ctx, p, s); break;
    }
    if (rc) return rc;
    if (out_set_mean) {
        double* sup = (double*)(base + p.o_sup);
        hipLaunchKernelGGL(k_dep_super_sums, dim3(p.supers, fd_cdiv(p.a.F, 256)), dim3(256), 0, s, p.a.part, p.a.chunks, p.a.F, sup);
        hipLaunchKernelGGL(k_dep_set_mean, dim3(fd_cdiv(p.a.F, 256)), dim3(256), 0, s, sup, p.supers, p.a.F, n, out_set_mean);
    }
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}
