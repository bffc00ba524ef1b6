// fd_signature.hip -- the truncated path signature of every series (NOT in the reference; Sig-W1 of Ni et al. 2021 and the signature
// MMD of Chevyrev & Oberhauser are host arithmetic on its outputs, utils/signature.py): the iterated integrals of the
// piecewise linear path through the points of a series up to depth m, their squared norm, and the mean of every entry over the set.
//
//   fd_series_signature     one fused kernel (k_signature) and a fixed-order, two-level reduction of the chunk sums
//
// The path.  p[t, c] = scale_c (x[t, c] - offset_c) in double; BASEPOINT prepends the point 0; increments D[s] = p[s + 1] - p[s] over
// Sb = T - 1 (T with a basepoint) segments; LEAD_LAG doubles the segments and the channels ([lead | lag]: segment 2 s moves the lead
// channels by D[s], segment 2 s + 1 the lag channels); TIME appends a channel that moves by 1 / S' per segment.  d letters, S' segments.
//
// The state of a series is its D = d + d^2 + ... + d^m doubles in the LDS, levels concatenated, a level row-major over its words (first
// letter slowest).  An ITEM is (series slot, word); a thread owns items tid, tid + G, ... (at most 8) for the whole launch and keeps
// their letters packed in registers.  Per segment, Chen's identity with the exponential of the linear segment in Horner form:
//     acc = D[w_1] / k;   acc = (acc + S_j[w_1..w_j]) D[w_{j+1}] / (k - j),  j = 1..k-1;   S_k[w] += acc
// Every thread reads (the state before the segment), a barrier, every owner adds its acc, a barrier.  A zero increment gives acc = 0 and
// leaves the state's bits alone; a letter whose channel has scale 0 makes every word that holds it an exact zero.  No product feeds an
// addition directly (and contraction is off for this file): p[s + 1] - p[s] of two equal points is exactly 0.
//
// Workgroup.  D <= 64: one wave, floor(64 / D) series side by side (ECG, d = 2, m = 4: D = 30, two series per wave; the barriers cost
// nothing).  Above that one series per workgroup of min(1024, D rounded up to 64) threads.  The series is staged in time tiles: the
// floats of a tile (plus one point) go to the LDS once, coalesced, the double increments are formed from them, and the segments run out
// of the LDS.  A series' values depend on that series, (T, C, depth, flags) and the offsets and scales alone.
//
// Set mean.  Series are cut into chunks of SIG_CHUNK = 32; a workgroup owns whole chunks.  The owner of word w (slot 0) adds the final
// state of the chunk's series in series order in double; the chunk sums go to work; k_sig_super_sums adds the chunks of every 64 in
// order and k_sig_set_mean those sums in order and divides by n.  The grouping depends on n alone: no atomics, bit-identical for every
// grid (FDIFF_SIG_SPLITS) and from run to run.  (The two small kernels restate fd_dependence.hip's: that file keeps its own in an
// anonymous namespace and is not touched here.)
#include <algorithm>
#include <cstdint>
#include <cstdlib>

#include "fd_pairs.h"

#pragma clang fp contract(off)

namespace {
using fdp::Carve;

constexpr int SIG_CHUNK = 32;         // series per partial sum of the set mean
constexpr int SIG_SUPER = 64;         // chunks per second-level partial sum
constexpr int SIG_MAX_T = 1024, SIG_MAX_C = 64, SIG_MAX_DEPTH = 6, SIG_MAX_D = 8192;
constexpr int SIG_STAGE = 4096;       // increments of a time tile, all slots together
constexpr int SIG_MAX_ROUNDS = 8;     // items per thread: SIG_MAX_D / 1024
constexpr size_t SIG_MAX_LDS = 160 * 1024;
constexpr int SIG_BASEPOINT = 1, SIG_LEAD_LAG = 2, SIG_TIME = 4;

struct SigArgs {
    const float* x;
    const double* offset;   // (C) or null
    const double* scale;    // (C) or null
    int n, T, C, depth, flags;
    int d, D;               // letters, features
    int Sb;                 // base segments: T - 1, T with a basepoint
    int spb;                // series slots of a workgroup
    int items;              // spb D
    int TT;                 // base segments per time tile
    int chunks, chunks_per_block;
    double tinc;            // 1 / S'
    float* sig;             // (n, D) or null
    double* sqnorm;         // (n) or null
    double* part;           // (chunks, D)
};

template <int R>
__global__ __launch_bounds__(1024) void k_signature(SigArgs g) {
    extern __shared__ double sig_smem[];
    const int C = g.C, d = g.d, D = g.D, G = blockDim.x, tid = threadIdx.x, spb = g.spb, Sb = g.Sb, TT = g.TT;
    const int bp = g.flags & SIG_BASEPOINT, ll = (g.flags & SIG_LEAD_LAG) ? 1 : 0, tch = (g.flags & SIG_TIME) ? d - 1 : -1;
    const int DS = TT * C, XS = (TT + 1) * C;
    double* state = sig_smem;                       // (spb, D)
    double* off = state + g.items;                  // (C)
    double* scl = off + C;                          // (C)
    double* red = scl + C;                          // (16) the waves' squared norms
    double* dbuf = red + 16;                        // (spb, TT, C) increments of the tile
    float* xbuf = (float*)(dbuf + (size_t)spb * DS);   // (spb, TT + 1, C) its points as they came

    for (int c = tid; c < C; c += G) {
        off[c] = g.offset ? g.offset[c] : 0.0;
        scl[c] = g.scale ? g.scale[c] : 1.0;
    }

    // the words of this thread's items: letter i in bits 8 i .., the level in bits 48..50, the slot from bit 52
    unsigned long long code[R];
    double cacc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int item = tid + r * G;
        code[r] = 0;
        cacc[r] = 0.0;
        if (item < g.items) {
            const int j = item / D;
            int q = item - j * D, k = 1, pw = d;
            while (q >= pw) { q -= pw; pw *= d; ++k; }
            unsigned long long cd = ((unsigned long long)k << 48) | ((unsigned long long)j << 52);
            for (int i = k - 1; i >= 0; --i) {
                const int l = q % d;
                q /= d;
                cd |= (unsigned long long)l << (8 * i);
            }
            code[r] = cd;
        }
    }
    __syncthreads();

    const size_t TC = (size_t)g.T * C;
    const int passes = (SIG_CHUNK + spb - 1) / spb;
    const int chunk_end = min(g.chunks, (int)(blockIdx.x + 1) * g.chunks_per_block);
    for (int chunk = blockIdx.x * g.chunks_per_block; chunk < chunk_end; ++chunk) {
        for (int pass = 0; pass < passes; ++pass) {
            const long long s_first = (long long)chunk * SIG_CHUNK + pass * spb;    // the series of slot 0
            const int live = (int)max(0ll, min((long long)min(spb, SIG_CHUNK - pass * spb), (long long)g.n - s_first));   // slots 0..live-1 hold a series
            if (live == 0) break;                                                  // the set's last chunk may be short
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int item = tid + r * G;
                if (item < g.items) state[item] = 0.0;
            }
            for (int s0 = 0; s0 < Sb; s0 += TT) {
                const int tt = min(TT, Sb - s0);
                // ---- the points s0 - bp .. s0 + tt - bp of every slot (row -1 is the basepoint: never read from memory)
                const int xn = (tt + 1) * C, first = (s0 - bp) * C;
                for (int e = tid; e < spb * xn; e += G) {
                    const int j = e / xn, i = e - j * xn;
                    float v = 0.f;
                    if (j < live && first + i >= 0) v = g.x[(size_t)(s_first + j) * TC + (size_t)(first + i)];
                    xbuf[j * XS + i] = v;
                }
                __syncthreads();
                const int dn = tt * C;
                for (int e = tid; e < spb * dn; e += G) {
                    const int j = e / dn, i = e - j * dn, c = i % C;
                    const float* xp = xbuf + j * XS + i;
                    const double pa = first + i >= 0 ? scl[c] * ((double)xp[0] - off[c]) : 0.0;
                    const double pb = scl[c] * ((double)xp[C] - off[c]);
                    dbuf[j * DS + i] = pb - pa;
                }
                __syncthreads();
                // ---- the segments of the tile
                for (int sg = 0; sg < (tt << ll); ++sg) {
                    const int s = sg >> ll, odd = sg & 1;
                    double acc[R];
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        acc[r] = 0.0;
                        const unsigned long long cd = code[r];
                        const int k = (int)(cd >> 48) & 7;
                        if (k) {
                            const int j = (int)(cd >> 52);
                            const double* Sj = state + j * D;
                            const double* dj = dbuf + j * DS + s * C;
                            auto delta = [&](int l) -> double {
                                if (l == tch) return g.tinc;
                                const int lag = l >= C;          // lead-lag only: without it every letter below tch is a channel
                                return (!ll || lag == odd) ? dj[lag ? l - C : l] : 0.0;
                            };
                            int l = (int)(cd & 0xff), p = l, lo = 0, pw = d;
                            double a = delta(l) / (double)k;
                            for (int jj = 1; jj < k; ++jj) {
                                l = (int)(cd >> (8 * jj)) & 0xff;
                                a = (a + Sj[lo + p]) * delta(l) / (double)(k - jj);
                                p = p * d + l;
                                lo += pw;
                                pw *= d;
                            }
                            acc[r] = a;
                        }
                    }
                    __syncthreads();
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const int item = tid + r * G;
                        if (item < g.items) state[item] += acc[r];
                    }
                    __syncthreads();
                }
            }
            // ---- the outputs of this pass
            double sq = 0.0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int item = tid + r * G;
                if (item < g.items) {
                    const int j = (int)(code[r] >> 52);
                    if (j < live) {
                        const double v = state[item];
                        if (g.sig) g.sig[(size_t)(s_first + j) * D + (item - j * D)] = (float)v;
                        sq += v * v;
                    }
                    if (item < D)
                        for (int jj = 0; jj < live; ++jj) cacc[r] += state[jj * D + item];
                }
            }
            if (g.sqnorm) {
                if (G == 64) {
                    // D <= 64: the thread of a slot's first word adds the slot's squares in word order
                    if (tid < g.items && tid % D == 0 && tid / D < live) {
                        double t = 0.0;
                        for (int w = 0; w < D; ++w) t += state[tid + w] * state[tid + w];
                        g.sqnorm[s_first + tid / D] = t;
                    }
                } else {
                    // one series: the thread's own squares in item order, a butterfly over the wave, the waves in order
                    for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
                    if ((tid & 63) == 0) red[tid >> 6] = sq;
                    __syncthreads();
                    if (tid == 0 && live) {
                        double t = 0.0;
                        for (int w = 0; w < (G >> 6); ++w) t += red[w];
                        g.sqnorm[s_first] = t;
                    }
                }
            }
            __syncthreads();
        }
        // ---- end of a chunk: every owner hands its sum over and starts again from zero
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int item = tid + r * G;
            if (item < D) {
                g.part[(size_t)chunk * D + item] = cacc[r];
                cacc[r] = 0.0;
            }
        }
    }
}

// The chunk sums are added in two fixed levels: level 1 adds the chunks of a super-chunk of SIG_SUPER chunks in chunk order, level 2
// the super-chunks in order and divides by n.  The loads of 16 terms are issued together, the additions stay in order.
__device__ __forceinline__ double sig_sum_in_order(const double* __restrict__ p, int count, size_t stride) {
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

__global__ __launch_bounds__(256) void k_sig_super_sums(const double* __restrict__ part, int chunks, int F, double* __restrict__ sup) {
    const int f = blockIdx.y * 256 + threadIdx.x, z0 = blockIdx.x * SIG_SUPER;
    if (f >= F) return;
    sup[(size_t)blockIdx.x * F + f] = sig_sum_in_order(part + (size_t)z0 * F + f, min(SIG_SUPER, chunks - z0), (size_t)F);
}

__global__ __launch_bounds__(256) void k_sig_set_mean(const double* __restrict__ sup, int supers, int F, int n, double* __restrict__ out) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    out[f] = sig_sum_in_order(sup + f, supers, (size_t)F) / (double)n;
}

// ---------------------------------------------------------------------------------------------- host side
struct SigPlan {
    SigArgs a;
    int G, R, grid, supers;
    size_t lds_bytes, o_part, o_sup, bytes;
};

// Everything but the grid is a function of (T, C, depth, flags); nothing a value depends on is a function of n or the grid.
int sig_plan(fd_ctx* ctx, const char* who, int n, int T, int C, int depth, int flags, SigPlan* out) {
    FD_REQUIRE(ctx, n >= 1 && T >= 2 && C >= 1, "%s: bad shape n=%d T=%d C=%d (n >= 1, T >= 2, C >= 1)", who, n, T, C);
    FD_REQUIRE(ctx, T <= SIG_MAX_T && C <= SIG_MAX_C, "%s: T=%d C=%d: at most T=%d and C=%d", who, T, C, SIG_MAX_T, SIG_MAX_C);
    FD_REQUIRE(ctx, depth >= 1 && depth <= SIG_MAX_DEPTH, "%s: depth=%d outside [1, %d]", who, depth, SIG_MAX_DEPTH);
    FD_REQUIRE(ctx, flags >= 0 && flags <= 7, "%s: flags=%d: bits 0 (basepoint), 1 (lead-lag) and 2 (time) only", who, flags);
    const int d = C * ((flags & SIG_LEAD_LAG) ? 2 : 1) + ((flags & SIG_TIME) ? 1 : 0);
    long long D = 0, pw = 1;
    for (int k = 1; k <= depth && D <= SIG_MAX_D; ++k) {
        pw *= d;
        D += pw;
    }
    FD_REQUIRE(ctx, D <= SIG_MAX_D, "%s: %d letters at depth %d give more than %d features: lower the depth", who, d, depth, SIG_MAX_D);
    FD_REQUIRE(ctx, (long long)n * D < (1ll << 31) && (long long)n * T * C < (1ll << 31),
               "%s: too large (n * D = %lld and n * T * C = %lld must stay below 2^31)", who, (long long)n * D, (long long)n * T * C);
    SigPlan p;
    SigArgs& a = p.a;
    a.n = n; a.T = T; a.C = C; a.depth = depth; a.flags = flags; a.d = d; a.D = (int)D;
    a.Sb = T - 1 + (flags & SIG_BASEPOINT);
    a.tinc = 1.0 / (double)(a.Sb * ((flags & SIG_LEAD_LAG) ? 2 : 1));
    p.G = std::min(1024, fd_cdiv(D, 64) * 64);
    a.spb = std::max(1, p.G / (int)D);
    a.items = a.spb * (int)D;
    const int rounds = fd_cdiv(a.items, p.G);
    p.R = rounds <= 1 ? 1 : rounds <= 2 ? 2 : rounds <= 4 ? 4 : SIG_MAX_ROUNDS;
    a.TT = std::max(1, std::min(a.Sb, SIG_STAGE / (a.spb * C)));
    p.lds_bytes = 8 * ((size_t)a.items + 2 * C + 16 + (size_t)a.spb * a.TT * C) + 4 * (size_t)a.spb * (a.TT + 1) * C;
    FD_REQUIRE(ctx, p.lds_bytes <= SIG_MAX_LDS, "%s: the plan needs %zu bytes of LDS, at most %zu", who, p.lds_bytes, SIG_MAX_LDS);
    a.chunks = fd_cdiv(n, SIG_CHUNK);
    // the grid: FDIFF_SIG_SPLITS workgroups (tests), else what the device holds at once (32 waves and 160 KiB of LDS per CU)
    const int per_cu = std::max(1, std::min(2048 / p.G, (int)(SIG_MAX_LDS / p.lds_bytes)));
    const char* e = getenv("FDIFF_SIG_SPLITS");
    const int forced = e ? atoi(e) : 0;
    const int want = std::max(1, std::min(a.chunks, forced > 0 ? forced : ctx->num_cu * per_cu));
    a.chunks_per_block = fd_cdiv(a.chunks, want);
    p.grid = fd_cdiv(a.chunks, a.chunks_per_block);
    p.supers = fd_cdiv(a.chunks, SIG_SUPER);
    Carve ws;
    p.o_part = ws.take((size_t)a.chunks * a.D * sizeof(double));
    p.o_sup = ws.take((size_t)p.supers * a.D * sizeof(double));
    p.bytes = ws.bytes();
    *out = p;
    return FD_OK;
}

template <int R>
int sig_launch(fd_ctx* ctx, const SigPlan& p, hipStream_t s) {
    static unsigned long long attr_set = 0;
    if (p.lds_bytes > 48 * 1024 && fd_first_on_device(attr_set, ctx->device))
        FD_HIP(ctx, hipFuncSetAttribute((const void*)k_signature<R>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SIG_MAX_LDS));
    hipLaunchKernelGGL(k_signature<R>, dim3(p.grid), dim3(p.G), p.lds_bytes, s, p.a);
    return FD_OK;
}

}  // namespace

extern "C" int fd_series_signature_workspace_bytes(fd_ctx* ctx, int n, int T, int C, int depth, int flags, size_t* bytes) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, bytes, "fd_series_signature_workspace_bytes: null pointer");
    SigPlan p;
    if (int rc = sig_plan(ctx, "fd_series_signature_workspace_bytes", n, T, C, depth, flags, &p)) return rc;
    *bytes = p.bytes;
    return FD_OK;
}

extern "C" int fd_series_signature(fd_ctx* ctx, const float* x, int n, int T, int C, int depth, int flags, const double* channel_offset,
                                   const double* channel_scale, float* sig, double* sqnorm, double* mean, void* work, size_t work_bytes,
                                   void* stream) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, x, "fd_series_signature: null x");
    SigPlan p;
    if (int rc = sig_plan(ctx, "fd_series_signature", n, T, C, depth, flags, &p)) return rc;
    FD_REQUIRE(ctx, mean, "fd_series_signature: null mean (the set mean is always written)");
    FD_REQUIRE(ctx, work && work_bytes >= p.bytes, "fd_series_signature: workspace of %zu bytes, fd_series_signature_workspace_bytes asks for %zu",
               work ? work_bytes : 0, p.bytes);
    hipStream_t s = (hipStream_t)stream;
    char* base = Carve::align(work);
    p.a.x = x;
    p.a.offset = channel_offset;
    p.a.scale = channel_scale;
    p.a.sig = sig;
    p.a.sqnorm = sqnorm;
    p.a.part = (double*)(base + p.o_part);
    int rc = FD_OK;
    switch (p.R) {
        case 1: rc = sig_launch<1>(ctx, p, s); break;
        case 2: rc = sig_launch<2>(ctx, p, s); break;
        case 4: rc = sig_launch<4>(ctx, p, s); break;
        default: rc = sig_launch<SIG_MAX_ROUNDS>(ctx, p, s); break;
    }
    if (rc) return rc;
    double* sup = (double*)(base + p.o_sup);
    hipLaunchKernelGGL(k_sig_super_sums, dim3(p.supers, fd_cdiv(p.a.D, 256)), dim3(256), 0, s, p.a.part, p.a.chunks, p.a.D, sup);
    hipLaunchKernelGGL(k_sig_set_mean, dim3(fd_cdiv(p.a.D, 256)), dim3(256), 0, s, sup, p.supers, p.a.D, n, mean);
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}
