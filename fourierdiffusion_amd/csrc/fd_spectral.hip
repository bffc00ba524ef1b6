// fd_spectral.hip -- how the channels of a series relate as a function of frequency (NOT in the reference; Welch's averaged
// periodogram with scipy.signal.welch / csd's conventions at fs = 1, scaling = "density", one-sided): per series the
// power spectral density of every channel, the cross-spectral density of every channel pair c < d and three summaries of each
// channel's spectrum, plus the mean of every feature over the set.
//
//   fd_series_spectra    one fused kernel (k_spectra) and a fixed-order, two-level reduction of the chunk sums
//
// A GROUP owns one series at a time -- one wave while a series is little work (at most 12 DFT tiles and 1024 cross-spectrum entries:
// one channel, or short segments), four to a workgroup, else the whole workgroup of 256 threads: it is read from HBM once into the LDS (raw, [t][c]) and everything else comes
// out of the LDS.  With S = nperseg, H = the hop, K = S / 2 + 1 bins and nseg segments, the COLUMNS of the series are its
// (segment, channel) pairs q = g C + c: every segment of every channel goes through ONE product.
//
//   segments        16 lanes share a column: each sums its strided entries in DOUBLE, a butterfly adds the 16 partial sums.  With
//                   detrend the entry is ((double)S x - sum) (1 / S): for floats on a grid (and for S equal floats) S x and the sum are
//                   exact, so the entry (times 1 / S in double) has the same bits for x and x + 1000, and is 0 for a constant
//                   channel.  It is multiplied by the DOUBLE window and rounded to f32 once, into the k-quad image V (Sp x Np).
//   DFT             F = Bt . V on v_mfma_f32_16x16x4_f32: Bt (Mp x Sp) holds cos(2 pi k s / S) in rows 0..K-1 and sin in rows K..2K-1,
//                   built on the device in double (the angle reduced as (k s mod S) / S first), rounded to f32 once and cached on the
//                   context per (S, window) with the double window in front of it; a workgroup copies it into the LDS once while the
//                   plan with it stays within 40 KiB, else it comes from the L2.  A 16 x 16 tile of F is one wave's; a column's
//                   arithmetic does not depend on the other columns.
//   cross-spectrum  an ENTRY is (k, c <= d); a thread owns entries e = its index in the group, + the group's size, ...: it adds conj(F_c) F_d over the segments in
//                   segment order in double (the products of two floats are exact in double), scales by scale_k / (nseg sum w^2)
//                   and rounds to f32.  The diagonal entries are the PSD and go through the same code: csd of a channel copied into
//                   two columns has the PSD's bits and imaginary part 0.
//   summaries       from the double PSD in the LDS: 16 lanes per channel, strided bins, butterfly.
//   set means       series are cut into chunks of SPEC_CHUNK = 32; a group owns whole chunks and every feature has ONE owner
//                   thread, which adds the f32 value as returned, in series order, into the feature's cell: in the LDS while F =
//                   K C + 2 K NP + 3 C doubles take 8 KiB or less (copied to part[chunk] at the end of the chunk), else part[chunk]
//                   itself (at 40 channels F is 167 KB: the L2 serves it, eight cells of a thread in flight together);
//                   k_spec_super_sums adds the chunks of every 64 in order and k_spec_set_mean those sums in order.  No atomics:
//                   bit-identical for every grid (FDIFF_SPEC_SPLITS) and from run to run.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "fd_pairs.h"
#include "fd_project.h"

namespace {
using fdp::Carve;
using fdproj::f32x4;

constexpr int SPEC_CHUNK = 32;       // series per partial sum of the set means
constexpr int SPEC_SUPER = 64;       // chunks per second-level partial sum
constexpr int SPEC_MAX_T = 1024, SPEC_MAX_C = 64;
constexpr int SPEC_THREADS = 256;
constexpr int SPEC_BATCH = 8;        // entries of the cross-spectrum a thread works on at once
constexpr int SPEC_PREFETCH = 4;     // floats of the next series a thread holds in registers while it works on this one
constexpr int SPEC_LANES = 16;       // lanes that share a column's mean / a channel's summaries
constexpr size_t SPEC_MAX_LDS = 160 * 1024;
constexpr size_t SPEC_BASIS_LDS = 40 * 1024; // the basis is staged in the LDS while the plan with it stays within this
constexpr int SPEC_WAVE_TILES = 12, SPEC_WAVE_ENTRIES = 1024;   // a series of at most this much work is one wave's
constexpr size_t SPEC_ACC_LDS = 8 * 1024;    // the chunk sums live in the LDS while they take no more than this

struct SpecArgs {
    const float* x;
    const double* win;      // (S) the window, double
    const float* basis;     // (Mp, Sp) row-major: cos rows 0..K-1, sin rows K..2K-1, zero outside (2K, S)
    int n, T, C, S, H, K, nseg, detrend;
    int NP;                 // C (C - 1) / 2
    int Sp, Mp, Np;         // S, 2 K and nseg C padded to 16
    int gsize;              // threads of a group: 64 while a series is little work, else the whole workgroup
    int o_pair, o_groups;   // byte offsets of the shared LDS pieces after the window: the pair table, the groups' own pieces
    int group_bytes;        // LDS of one group
    int o_v, o_f, o_pd;     // byte offsets of a group's pieces after its series
    int o_acc;              // of the chunk sums' cells while F doubles are few, or -1: the cells are part[chunk] itself
    int prefetch;           // the next series fits the prefetch registers
    int o_basis;            // of the LDS copy of the basis (row stride Sp + 4: conflict-free 16-byte reads), or -1: read it from the L2
    int chunks, chunks_per_group;
    int F;                  // features of the set mean
    double norm;            // 1 / (nseg sum w^2)
    double inv_log_bins;    // 1 / ln(K - 1), 0 for K = 2
    float* out_psd;         // (n, K, C) or null
    float* out_csd;         // (n, K, NP, 2) or null
    float* out_sum;         // (n, C, 3) or null
    double* part;           // (chunks, F)
};

__device__ __forceinline__ double spec_butterfly(double v) {
#pragma unroll
    for (int o = SPEC_LANES >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// 16 rows of the row-major basis M (Sp columns, a multiple of 16, at row stride `stride`) times 16 columns of the k-quad image V (Np
// columns; V points at the tile's first column): fdproj::tile_product with the image's width as an argument.  The lane (li, kq) loads four consecutive k
// of its row and of its column at once and feeds them to four MFMAs, so MFMA i of a step sums k = k0 + i, k0 + 4 + i, k0 + 8 + i,
// k0 + 12 + i in that order; two accumulators (i even / odd) hide the dependent latency.  Returns rows row0 + 4 kq .. + 3 of column li.
__device__ __forceinline__ f32x4 spec_tile_product(const float* __restrict__ M, int row0, int stride, int Sp, const float* V, int Np, int li,
                                                   int kq) {
    const float* arow = M + (size_t)(row0 + li) * stride + 4 * kq;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < Sp; k0 += 16) {
        const f32x4 av = *reinterpret_cast<const f32x4*>(arow + k0);
        const f32x4 bv = *reinterpret_cast<const f32x4*>(V + ((size_t)(k0 / 4 + kq) * Np + li) * 4);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[0], bv[0], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[1], bv[1], acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[2], bv[2], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[3], bv[3], acc1, 0, 0, 0);
    }
    return acc0 + acc1;
}

// owner-thread accumulation of a chunk's sum: the first series of a chunk starts the cell
__device__ __forceinline__ void spec_add(double* cell, float v, bool first) { *cell = first ? (double)v : *cell + (double)v; }

__global__ __launch_bounds__(SPEC_THREADS) void k_spectra(SpecArgs g) {
    extern __shared__ double spec_smem[];
    const int T = g.T, C = g.C, S = g.S, K = g.K, NP = g.NP, Np = g.Np, nseg = g.nseg, TC = T * C, gsz = g.gsize;
    const int tid = threadIdx.x, grp = tid / gsz, gtid = tid - grp * gsz, gpb = SPEC_THREADS / gsz;
    const int lane = tid & 63, gwave = gtid >> 6, gwaves = gsz >> 6;
    // shared by the groups: the window, the pair table and (if staged) the basis; then every group's own pieces
    char* shared = (char*)spec_smem;
    double* wl = (double*)shared;                           // (S) the window
    unsigned char* pair_c = (unsigned char*)(shared + g.o_pair);
    unsigned char* pair_d = pair_c + NP;
    float* Bl = (float*)(shared + (g.o_basis >= 0 ? g.o_basis : 0));
    char* base = shared + g.o_groups + (size_t)grp * g.group_bytes;
    float* xs = (float*)base;                               // (T, C) the series as it lies in memory
    float* V = (float*)(base + g.o_v);                      // (Sp / 4, Np, 4) the centred, windowed segments, k-quad order
    float* Fi = (float*)(base + g.o_f);                     // (Mp, Np) the DFT: cos sums, then sin sums
    double* Pd = (double*)(base + g.o_pd);                  // (K, C) the PSD of the current series, double
    double* acc = (double*)(base + (g.o_acc >= 0 ? g.o_acc : 0));   // (F) the chunk sums, if they live here

    for (int i = gtid; i < g.Sp * Np; i += gsz) V[i] = 0.f;               // the padding stays zero: only live entries are rewritten
    for (int i = tid; i < S; i += SPEC_THREADS) wl[i] = g.win[i];
    if (g.o_basis >= 0)
        for (int i = tid; i < g.Mp * g.Sp; i += SPEC_THREADS) Bl[(i / g.Sp) * (g.Sp + 4) + i % g.Sp] = g.basis[i];
    for (int c = tid; c < C - 1; c += SPEC_THREADS) {
        int p = c * C - c * (c + 1) / 2;                                  // pairs before row c
        for (int d = c + 1; d < C; ++d, ++p) {
            pair_c[p] = (unsigned char)c;
            pair_d[p] = (unsigned char)d;
        }
    }
    __syncthreads();

    const int CP = C + NP, E = K * CP, ncol = nseg * C;
    const int p16 = tid & (SPEC_LANES - 1);
    const double Sd = (double)S, inv_S = 1.0 / Sd;
    const size_t csd_off = (size_t)K * C, sum_off = csd_off + (size_t)2 * K * NP;
    const int chunk0 = (blockIdx.x * gpb + grp) * g.chunks_per_group;
    const int nslots = g.chunks_per_group * SPEC_CHUNK;     // the same for every group: the barriers below are uniform

    float pre[SPEC_PREFETCH];
    bool have_pre = false;
    for (int slot = 0; slot < nslots; ++slot) {
        const int chunk = chunk0 + slot / SPEC_CHUNK;
        const long long s = (long long)chunk * SPEC_CHUNK + slot % SPEC_CHUNK;
        const bool live = chunk < g.chunks && s < g.n;
        const bool first = slot % SPEC_CHUNK == 0;
        double* part = g.o_acc >= 0 ? acc : g.part + (size_t)min(chunk, g.chunks - 1) * g.F;

        if (live) {
            if (have_pre) {
#pragma unroll
                for (int k = 0; k < SPEC_PREFETCH; ++k) {
                    const int i = gtid + k * gsz;
                    if (i < TC) xs[i] = pre[k];
                }
            } else {
                const float* xg = g.x + (size_t)s * TC;
                for (int i = gtid; i < TC; i += gsz) xs[i] = xg[i];
            }
        }
        __syncthreads();

        // ---- segments: lane p16 of the 16 lanes of column q = (seg, c) takes s = p16, p16 + 16, ...
        if (live) {
            for (int q = gtid / SPEC_LANES; q < ncol; q += gsz / SPEC_LANES) {
                const int seg = q / C, c = q - seg * C;
                const float* col = xs + (size_t)seg * g.H * C + c;
                double sum = 0.0;
                if (g.detrend) {
                    for (int i = p16; i < S; i += SPEC_LANES) sum += (double)col[i * C];
                    sum = spec_butterfly(sum);
                }
                for (int i = p16; i < S; i += SPEC_LANES) {
                    const double xv = (double)col[i * C];
                    const double e = g.detrend ? (Sd * xv - sum) * inv_S : xv;
                    V[((i >> 2) * Np + q) * 4 + (i & 3)] = (float)(e * wl[i]);
                }
            }
        }
        __syncthreads();

        // ---- the next series travels while this one is multiplied
        have_pre = false;
        if (g.prefetch && slot + 1 < nslots) {
            const int nchunk = chunk0 + (slot + 1) / SPEC_CHUNK;
            const long long ns = (long long)nchunk * SPEC_CHUNK + (slot + 1) % SPEC_CHUNK;
            if (nchunk < g.chunks && ns < g.n) {
                const float* xn = g.x + (size_t)ns * TC;
#pragma unroll
                for (int k = 0; k < SPEC_PREFETCH; ++k) {
                    const int i = gtid + k * gsz;
                    pre[k] = i < TC ? xn[i] : 0.f;
                }
                have_pre = true;
            }
        }

        // ---- DFT: tile (jt, qt) of F = Bt . V; lane (li, kq) holds rows 4 kq .. 4 kq + 3 of column li of the tile
        if (live) {
            const int li = lane & 15, kq = lane >> 4, qtiles = Np / 16, tiles = (g.Mp / 16) * qtiles;
            for (int t = gwave; t < tiles; t += gwaves) {
                const int jt = t / qtiles, qt = t - jt * qtiles;
                const f32x4 a4 = g.o_basis >= 0 ? spec_tile_product(Bl, jt * 16, g.Sp + 4, g.Sp, V + (size_t)qt * 64, Np, li, kq)
                                                : spec_tile_product(g.basis, jt * 16, g.Sp, g.Sp, V + (size_t)qt * 64, Np, li, kq);
#pragma unroll
                for (int r = 0; r < 4; ++r) Fi[(jt * 16 + 4 * kq + r) * Np + qt * 16 + li] = a4[r];
            }
        }
        __syncthreads();

        // ---- cross-spectrum: entry e = (k, r); r < C the diagonal (c, c), else pair r - C.  Eight entries at a time: the eight cells'
        // loads are in flight together (one at a time, 42 dependent round trips to the L2 per series at 40 channels)
        for (int e0 = gtid; live && e0 < E; e0 += SPEC_BATCH * gsz) {
            float vr[SPEC_BATCH], vi[SPEC_BATCH];
            size_t cell[SPEC_BATCH];
            bool ok[SPEC_BATCH], two[SPEC_BATCH];
#pragma unroll
            for (int j = 0; j < SPEC_BATCH; ++j) {
                const int e = e0 + j * gsz;
                ok[j] = e < E;
                two[j] = false;
                cell[j] = 0;
                vr[j] = vi[j] = 0.f;
                if (!ok[j]) continue;
                const int k = e / CP, r = e - k * CP;
                const int c = r < C ? r : pair_c[r - C], d = r < C ? r : pair_d[r - C];
                const float* fa = Fi + (size_t)k * Np;
                const float* fb = Fi + (size_t)(K + k) * Np;
                double re = 0.0, im = 0.0;
                for (int seg = 0; seg < nseg; ++seg) {
                    const double ac = (double)fa[seg * C + c], bc = (double)fb[seg * C + c];
                    const double ad = (double)fa[seg * C + d], bd = (double)fb[seg * C + d];
                    re = fma(ac, ad, re);                                 // F = A - i B: conj(F_c) F_d = A_c A_d + B_c B_d + i (B_c A_d - A_c B_d)
                    re = fma(bc, bd, re);
                    im += fma(bc, ad, -(ac * bd));                        // both products are exact in double: 0 for equal columns
                }
                const double scale = (k == 0 || 2 * k == S) ? g.norm : 2.0 * g.norm;
                re *= scale;
                im *= scale;
                vr[j] = (float)re;
                vi[j] = (float)im;
                if (r < C) {
                    Pd[k * C + c] = re;
                    if (g.out_psd) g.out_psd[((size_t)s * K + k) * C + c] = vr[j];
                    cell[j] = (size_t)k * C + c;
                } else {
                    const size_t o = ((size_t)k * NP + (r - C)) * 2;
                    if (g.out_csd) {
                        float* dst = g.out_csd + (size_t)s * K * NP * 2 + o;
                        dst[0] = vr[j];
                        dst[1] = vi[j];
                    }
                    two[j] = true;
                    cell[j] = csd_off + o;
                }
            }
            double o0[SPEC_BATCH], o1[SPEC_BATCH];
#pragma unroll
            for (int j = 0; j < SPEC_BATCH; ++j) {
                o0[j] = (ok[j] && !first) ? part[cell[j]] : 0.0;
                o1[j] = (two[j] && !first) ? part[cell[j] + 1] : 0.0;
            }
#pragma unroll
            for (int j = 0; j < SPEC_BATCH; ++j) {
                if (ok[j]) part[cell[j]] = first ? (double)vr[j] : o0[j] + (double)vr[j];
                if (two[j]) part[cell[j] + 1] = first ? (double)vi[j] : o1[j] + (double)vi[j];
            }
        }
        __syncthreads();

        // ---- summaries: lane p16 of the 16 lanes of channel c takes bins 1 + p16, 17 + p16, ...; bin 0 enters the total power alone
        if (live) {
            for (int c = gtid / SPEC_LANES; c < C; c += gsz / SPEC_LANES) {
                double tot = 0.0, num = 0.0;
                for (int k = 1 + p16; k < K; k += SPEC_LANES) {
                    const double p = Pd[k * C + c];
                    tot += p;
                    num += (double)k * p;
                }
                tot = spec_butterfly(tot);
                num = spec_butterfly(num);
                double ent = 0.0;
                if (tot > 0.0) {
                    const double inv_tot = 1.0 / tot;
                    for (int k = 1 + p16; k < K; k += SPEC_LANES) {
                        const double p = Pd[k * C + c] * inv_tot;
                        if (p > 0.0) ent -= p * log(p);
                    }
                }
                ent = spec_butterfly(ent);
                if (p16 == 0) {
                    const float sm[3] = {(float)(tot + Pd[c]), tot > 0.0 ? (float)(num / (tot * Sd)) : 0.f,
                                         tot > 0.0 ? (float)(ent * g.inv_log_bins) : 0.f};
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        if (g.out_sum) g.out_sum[((size_t)s * C + c) * 3 + i] = sm[i];
                        spec_add(part + sum_off + (size_t)c * 3 + i, sm[i], first);
                    }
                }
            }
        }
        // ---- end of a chunk: cells that live in the LDS go to part[chunk] (a short last chunk waits for slot 31 too: the dead slots
        // touch nothing); the next series' barriers stand between this and the cells' next use, as between the reads of Pd / Fi above
        // and their next writes
        if (g.o_acc >= 0 && slot % SPEC_CHUNK == SPEC_CHUNK - 1) {
            __syncthreads();
            if (chunk < g.chunks)
                for (int f = gtid; f < g.F; f += gsz) g.part[(size_t)chunk * g.F + f] = acc[f];
        }
    }
}

// the window (S doubles) and the basis (Mp x Sp floats) of one (S, window): double arithmetic, the angle reduced in integers first
__global__ __launch_bounds__(256) void k_spec_tables(double* __restrict__ win, float* __restrict__ basis, int S, int K, int Sp, int Mp,
                                                     int window) {
    const double two_pi = 6.283185307179586476925286766559;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < Sp) win[i] = i < S ? (window == 1 ? 0.5 - 0.5 * cos(two_pi * (double)i / (double)S) : 1.0) : 0.0;
    if (i >= Mp * Sp) return;
    const int j = i / Sp, t = i - j * Sp;
    float v = 0.f;
    if (j < 2 * K && t < S) {
        const int k = j < K ? j : j - K;
        const double a = two_pi * (double)((k * t) % S) / (double)S;
        v = (float)(j < K ? cos(a) : sin(a));
    }
    basis[i] = v;
}

// The chunk sums are added in two fixed levels, as fd_dependence.hip does: level 1 adds the chunks of a super-chunk of SPEC_SUPER = 64
// chunks in chunk order, level 2 the super-chunks in order and divides by n.  The grouping depends on n alone.
__device__ __forceinline__ double spec_sum_in_order(const double* __restrict__ p, int count, size_t stride) {
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

__global__ __launch_bounds__(256) void k_spec_super_sums(const double* __restrict__ part, int chunks, int F, double* __restrict__ sup) {
    const int f = blockIdx.y * 256 + threadIdx.x, z0 = blockIdx.x * SPEC_SUPER;
    if (f >= F) return;
    sup[(size_t)blockIdx.x * F + f] = spec_sum_in_order(part + (size_t)z0 * F + f, min(SPEC_SUPER, chunks - z0), (size_t)F);
}

__global__ __launch_bounds__(256) void k_spec_set_mean(const double* __restrict__ sup, int supers, int F, int n, double* __restrict__ out) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    out[f] = spec_sum_in_order(sup + f, supers, (size_t)F) / (double)n;
}

// ---------------------------------------------------------------------------------------------- host side
struct SpecPlan {
    SpecArgs a;
    int grid, supers, window;
    size_t lds_bytes, o_part, o_sup, bytes;
};

size_t spec_round16(size_t b) { return (b + 15) & ~(size_t)15; }

// Everything but the grid is a function of the shape and the segment arguments; a value depends on nothing but (T, C, S, H, window,
// detrend).
int spec_plan(fd_ctx* ctx, const char* who, int n, int T, int C, int S, int noverlap, int window, int detrend, SpecPlan* out) {
    FD_REQUIRE(ctx, n >= 1 && T >= 1 && C >= 1, "%s: bad shape n=%d T=%d C=%d (all >= 1)", who, n, T, C);
    FD_REQUIRE(ctx, T <= SPEC_MAX_T && C <= SPEC_MAX_C, "%s: T=%d C=%d: at most T=%d and C=%d", who, T, C, SPEC_MAX_T, SPEC_MAX_C);
    FD_REQUIRE(ctx, S >= 2 && S <= T, "%s: nperseg=%d outside [2, T = %d]", who, S, T);
    FD_REQUIRE(ctx, noverlap >= 0 && noverlap <= S - 1, "%s: noverlap=%d outside [0, nperseg - 1 = %d]", who, noverlap, S - 1);
    FD_REQUIRE(ctx, window == 0 || window == 1, "%s: window=%d is neither 0 (boxcar) nor 1 (hann)", who, window);
    FD_REQUIRE(ctx, detrend == 0 || detrend == 1, "%s: detrend=%d is neither 0 (none) nor 1 (constant)", who, detrend);
    SpecPlan p;
    SpecArgs& a = p.a;
    a.n = n; a.T = T; a.C = C; a.S = S; a.H = S - noverlap; a.K = S / 2 + 1; a.detrend = detrend;
    a.nseg = (T - S) / a.H + 1;
    a.NP = C * (C - 1) / 2;
    a.Sp = fd_cdiv(S, 16) * 16;
    a.Mp = fd_cdiv(2 * a.K, 16) * 16;
    a.Np = fd_cdiv((long long)a.nseg * C, 16) * 16;
    const long long F = (long long)a.K * C + 2ll * a.K * a.NP + 3ll * C;
    FD_REQUIRE(ctx, (long long)n * F < (1ll << 31) && (long long)n * T * C < (1ll << 31),
               "%s: too large (n * F = %lld and n * T * C = %lld must stay below 2^31)", who, (long long)n * F, (long long)n * T * C);
    a.F = (int)F;
    // the LDS: shared by the groups of a workgroup the window, the pair table and (below) the basis; per series (per group) the series,
    // the segment image, the DFT image, the double PSD and (while they are few) the chunk sums' cells
    const size_t b_x = spec_round16((size_t)T * C * 4), b_v = (size_t)a.Sp * a.Np * 4, b_f = (size_t)a.Mp * a.Np * 4,
                 b_pd = spec_round16((size_t)a.K * C * 8), b_pair = spec_round16((size_t)2 * a.NP), b_win = (size_t)a.Sp * 8;
    size_t group = b_x + b_v + b_f + b_pd;
    a.o_v = (int)b_x;
    a.o_f = (int)(b_x + b_v);
    a.o_pd = (int)(b_x + b_v + b_f);
    a.o_acc = -1;
    if ((size_t)a.F * 8 <= SPEC_ACC_LDS) {
        a.o_acc = (int)group;
        group += spec_round16((size_t)a.F * 8);
    }
    size_t shared = b_win + b_pair;
    FD_REQUIRE(ctx, shared + group <= SPEC_MAX_LDS,
               "%s: T=%d C=%d nperseg=%d noverlap=%d needs %zu bytes of LDS per series (the series, and %d segments x %d channels "
               "of %d points and of %d DFT rows), at most %zu: ask for fewer segments (less overlap) or a shorter nperseg",
               who, T, C, S, noverlap, shared + group, a.nseg, C, a.Sp, a.Mp, SPEC_MAX_LDS);
    a.o_pair = (int)b_win;
    // a wave per series while a series is little work (few DFT tiles, few cross-spectrum entries) and four of them fit; else the workgroup
    const long long tiles = (long long)(a.Mp / 16) * (a.Np / 16), entries = (long long)a.K * (C + a.NP);
    a.gsize = (tiles <= SPEC_WAVE_TILES && entries <= SPEC_WAVE_ENTRIES && shared + 4 * group <= SPEC_MAX_LDS) ? 64 : SPEC_THREADS;
    const int gpb = SPEC_THREADS / a.gsize;
    a.group_bytes = (int)group;
    a.prefetch = T * C <= SPEC_PREFETCH * a.gsize ? 1 : 0;
    // the basis comes into the LDS too while the whole plan with it stays within 40 KiB (four workgroups a CU keep theirs); else the L2
    // serves it
    const size_t b_basis = (size_t)a.Mp * (a.Sp + 4) * 4;
    a.o_basis = -1;
    if (shared + b_basis + gpb * group <= SPEC_BASIS_LDS) {
        a.o_basis = (int)shared;
        shared += b_basis;
    }
    a.o_groups = (int)shared;
    const size_t lds = shared + gpb * group;
    p.lds_bytes = lds;
    p.window = window;
    double sw2 = 0.0;
    for (int i = 0; i < S; ++i) {
        const double w = window == 1 ? 0.5 - 0.5 * cos(6.283185307179586476925286766559 * (double)i / (double)S) : 1.0;
        sw2 += w * w;
    }
    a.norm = 1.0 / ((double)a.nseg * sw2);
    a.inv_log_bins = a.K > 2 ? 1.0 / log((double)(a.K - 1)) : 0.0;
    a.chunks = fd_cdiv(n, SPEC_CHUNK);
    // the grid: FDIFF_SPEC_SPLITS workgroups (tests), else ONE chunk per group: a group works through its 32 series one after the other,
    // each a chain of dependent steps, so a second chunk doubles its time, while a workgroup beyond what the device holds at once
    // starts as soon as another ends
    const char* e = getenv("FDIFF_SPEC_SPLITS");
    const int forced = e ? atoi(e) : 0;
    const int most = fd_cdiv(a.chunks, gpb);
    const int want = std::max(1, std::min(most, forced > 0 ? forced : most));
    a.chunks_per_group = fd_cdiv(a.chunks, want * gpb);
    p.grid = fd_cdiv(a.chunks, a.chunks_per_group * gpb);
    p.supers = fd_cdiv(a.chunks, SPEC_SUPER);
    Carve ws;
    p.o_part = ws.take((size_t)a.chunks * a.F * sizeof(double));
    p.o_sup = ws.take((size_t)p.supers * a.F * sizeof(double));
    p.bytes = ws.bytes();
    *out = p;
    return FD_OK;
}

// the cached window and basis of (S, window): ctx->fft_tw under a key below every other table's (fd_project.h lists them)
const float* spec_tables(fd_ctx* ctx, const SpecArgs& a, int window, hipStream_t s) {
    const size_t n = (size_t)2 * a.Sp + (size_t)a.Mp * a.Sp;
    return fdproj::cached_table(ctx, -(8 << 20) - (2 * a.S + window), n, s, [&](float* tab) {
        hipLaunchKernelGGL(k_spec_tables, dim3(fd_cdiv((long long)a.Mp * a.Sp, 256)), dim3(256), 0, s, (double*)tab, tab + 2 * a.Sp, a.S,
                           a.K, a.Sp, a.Mp, window);
    });
}

}  // namespace

extern "C" int fd_series_spectra_workspace_bytes(fd_ctx* ctx, int n, int T, int C, int nperseg, int noverlap, size_t* bytes) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, bytes, "fd_series_spectra_workspace_bytes: null pointer");
    SpecPlan p;
    if (int rc = spec_plan(ctx, "fd_series_spectra_workspace_bytes", n, T, C, nperseg, noverlap, 0, 0, &p)) return rc;
    *bytes = p.bytes;
    return FD_OK;
}

extern "C" int fd_series_spectra(fd_ctx* ctx, const float* x, int n, int T, int C, int nperseg, int noverlap, int window, int detrend,
                                 float* out_psd, float* out_csd, float* out_summary, double* out_set_mean, void* work, size_t work_bytes,
                                 void* stream) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, x, "fd_series_spectra: null x");
    SpecPlan p;
    if (int rc = spec_plan(ctx, "fd_series_spectra", n, T, C, nperseg, noverlap, window, detrend, &p)) return rc;
    FD_REQUIRE(ctx, out_set_mean, "fd_series_spectra: null out_set_mean (the set mean is always computed)");
    FD_REQUIRE(ctx, !out_csd || C >= 2, "fd_series_spectra: out_csd with C=1 (no pairs)");
    FD_REQUIRE(ctx, work && work_bytes >= p.bytes, "fd_series_spectra: workspace of %zu bytes, fd_series_spectra_workspace_bytes asks for %zu",
               work ? work_bytes : 0, p.bytes);
    hipStream_t s = (hipStream_t)stream;
    const float* tab = spec_tables(ctx, p.a, window, s);
    if (!tab) return fd_fail(ctx, FD_ERR_HIP, "fd_series_spectra: the basis of nperseg=%d could not be built", nperseg);
    p.a.x = x;
    p.a.win = (const double*)tab;
    p.a.basis = tab + 2 * p.a.Sp;
    p.a.out_psd = out_psd;
    p.a.out_csd = out_csd;
    p.a.out_sum = out_summary;
    char* base = Carve::align(work);
    p.a.part = (double*)(base + p.o_part);
    static unsigned long long attr_set = 0;
    if (p.lds_bytes > 48 * 1024 && fd_first_on_device(attr_set, ctx->device))
        FD_HIP(ctx, hipFuncSetAttribute((const void*)k_spectra, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SPEC_MAX_LDS));
    hipLaunchKernelGGL(k_spectra, dim3(p.grid), dim3(SPEC_THREADS), p.lds_bytes, s, p.a);
    double* sup = (double*)(base + p.o_sup);
    hipLaunchKernelGGL(k_spec_super_sums, dim3(p.supers, fd_cdiv(p.a.F, 256)), dim3(256), 0, s, p.a.part, p.a.chunks, p.a.F, sup);
    hipLaunchKernelGGL(k_spec_set_mean, dim3(fd_cdiv(p.a.F, 256)), dim3(256), 0, s, sup, p.supers, p.a.F, n, out_set_mean);
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}
