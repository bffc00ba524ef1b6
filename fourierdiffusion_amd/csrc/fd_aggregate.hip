// fd_aggregate.hip -- conditional sampling on window-mean observations (NOT in the reference): temporal super-resolution,
// disaggregation and forecasting from a series reported at a coarser rate than the model's.  The coordinate mask of fd_impute.hip and
// fd_dps.hip becomes a linear observation operator.  With w the window length, J = ceil(T / w) windows, window j = [j w,
// min((j + 1) w, T)) of length l_j (the last one may be short), per channel:
//
//   (P v)_j   = (1 / l_j) sum_{t in window j} v_t     (J x T, the window means)
//   (P^+ r)_t = r_{j(t)}                               (the broadcast; P P^+ = I)
//   (P^T r)_t = r_{j(t)} / l_{j(t)}
//
// m (J,C) masks windows, y (J,C) holds window means at data scale and x0_obs = A^-1(P^+ where(m, y, 0)), A(x) = idft(sigma x + mu).
// Replacement (Song et al. 2021 for a general linear observation: the orthogonal projector P^+ P in the place of the mask), d as in
// fd_impute.hip:
//   x' = x + dft(P^+ (m . P idft(sigma . d))) / sigma          (fourier = 0: x' = x + P^+ (m . P (sigma . d)) / sigma)
// Guidance (fd_dps.hip's derivation with the residual of the window means):
//   r = m . P idft(sigma . (x0_obs - x0_hat))   (J,C)          (fourier = 0: m . P (sigma . (x0_obs - x0_hat)))
//   u = sigma . diag(1/rho) F P^T r                              (fourier = 0: sigma . P^T r)
// sigma varies inside a window, so it no longer cancels in the time domain: both domains read it.
//
// Fourier path: idft = F^T diag(1/rho), so P idft(v) = (P F^T)(v / rho) and dft(P^+ R) = (F P^+) R: two RECTANGULAR bases per
// (T, w), A_w = P F^T (Jp x Tp) and B_w = F P^+ (Tp x Jp), Jp = 16 ceil(J / 16), built once on the device in double, rounded to f32
// and cached on the context.  F P^T = F P^+ diag(1 / l): the guidance divides the J masked means by l_j and reads the same B_w.
// One 512-thread workgroup per (row, block of 16 channels).  Phase 1 is that of the mask kernels (same Philox groups and counters):
// sigma d / rho into the k-quad LDS image U (Tp x 16).  Phase 2: R = A_w U (v_mfma_f32_16x16x4_f32, 16 windows x 16 channels per
// tile, the window tiles dealt over the 8 waves), masked per window into the k-quad image R (Jp x 16).  Phase 3: Y = B_w R over the
// T packed rows.  Both products are J/T of the mask path's.  LDS = 64 (Tp + Jp) bytes.
// Time-domain path: sigma d goes to an LDS time image (T x 16); one thread per (window, channel) sums its window in ascending t and
// writes the masked mean back over the window.  Every sum runs in a fixed order: two runs are bit-identical.
#include <algorithm>
#include <cmath>

#include "fd_aggregate.h"
#include "fd_philox.h"

namespace {

constexpr int kThreads = 512;    // 8 waves: the row tiles of a product are dealt round-robin
constexpr int kCB = 16;          // channels per workgroup = N of the MFMA tile

typedef __attribute__((ext_vector_type(4))) float f32x4;

__device__ __forceinline__ float inv_r(int k, int T) { return (k == 0 || (2 * k == T)) ? 1.0f : 2.0f; }
__device__ __forceinline__ int quad_idx(int k, int c) { return ((k >> 2) * kCB + c) * 4 + (k & 3); }
__device__ __forceinline__ int win_len(int j, int w, int T) { return min(w, T - j * w); }

// acc = M[row0 + li][0 .. K) . V[0 .. K)[li-th channel]: M row-major with row stride K (a multiple of 16), V a k-quad LDS image
__device__ __forceinline__ f32x4 tile_product(const float* __restrict__ M, int row0, int K, const float* V, int li, int kq) {
    const float* arow = M + (size_t)(row0 + li) * K + 4 * kq;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += 16) {
        const f32x4 av = *reinterpret_cast<const f32x4*>(arow + k0);
        const f32x4 bv = *reinterpret_cast<const f32x4*>(V + ((k0 / 4 + kq) * kCB + li) * 4);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[0], bv[0], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[1], bv[1], acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[2], bv[2], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[3], bv[3], acc1, 0, 0, 0);
    }
    return acc0 + acc1;
}

template <bool STEP, bool FOURIER>
__global__ __launch_bounds__(kThreads) void k_impute_agg(fd_agg_imp_args a) {
    extern __shared__ float lds[];
    float* U = lds;                            // FOURIER: sigma d / rho, frequency rows (k-quad); else sigma d, time rows [t][channel]
    float* R = lds + (size_t)a.Tp * kCB;       // FOURIER: m . P idft(sigma d), window rows (k-quad)
    const int tid = threadIdx.x;
    const int b = blockIdx.x / a.ncb, c0 = (blockIdx.x % a.ncb) * kCB;
    const int T = a.T, C = a.C, Tp = a.Tp, J = a.p.J, Jp = a.p.Jp, w = a.p.window;
    const size_t TC = (size_t)T * C, base = (size_t)b * TC, obase = (size_t)(b / a.obs_rep) * TC;
    const uint8_t* mrow = a.mask + (a.mask_per_series ? (size_t)(b / a.obs_rep) * J * C : 0);

    if (FOURIER) {
        for (int i = tid; i < Tp * kCB; i += kThreads) U[i] = 0.f;
        __syncthreads();
    }

    // ---- phase 1: step + d, over the Philox groups that touch this series (k_impute's: a group straddling two series is drawn by both)
    const size_t g_lo = base / 4, g_hi = (base + TC + 3) / 4;
    for (size_t g = g_lo + tid; g < g_hi; g += kThreads) {
        int loc[4];
        bool own[4], any = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const size_t e = g * 4 + j;
            own[j] = false;
            loc[j] = 0;
            if (e >= base && e < base + TC) {
                loc[j] = (int)(e - base);
                const int c = loc[j] % C;
                own[j] = c >= c0 && c < c0 + kCB;
            }
            any |= own[j];
        }
        if (!any) continue;
        float zs[4] = {0.f, 0.f, 0.f, 0.f}, zo[4] = {0.f, 0.f, 0.f, 0.f};
        if (STEP) {
            if (a.zstep) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (own[j]) zs[j] = a.zstep[base + loc[j]];
            } else {
                fd_randn4(a.off_step + g, a.seed, zs);
            }
        }
        if (a.s != 0.f) {        // the hard projection (s = 0) reads no observation noise
            if (a.zobs) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (own[j]) zo[j] = a.zobs[base + loc[j]];
            } else {
                fd_randn4(a.off_obs + g, a.seed, zo);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!own[j]) continue;
            const size_t e = base + loc[j];
            const int t = loc[j] / C, c = loc[j] % C;
            const float Gt = a.G[t];
            float xv = a.x[e];
            if (STEP) xv = fd_sde_apply(xv, a.score[e], zs[j], Gt, a.cf);
            const float xo = a.alpha * a.x0[obase + loc[j]] + a.s * (Gt * zo[j]);
            const float sd = a.stdv ? a.stdv[(size_t)t * C + c] : 1.0f;
            a.out[e] = xv;
            if (FOURIER) U[quad_idx(t, c - c0)] = sd * (xo - xv) * inv_r(t, T);
            else U[t * kCB + (c - c0)] = sd * (xo - xv);
        }
    }
    __syncthreads();     // U complete; out holds x_new (workgroup-scope release / acquire covers the global stores)

    if (!FOURIER) {
        // ---- one thread per (window, channel): the mean in ascending t, masked, written back over the window
        for (int i = tid; i < J * kCB; i += kThreads) {
            const int j = i / kCB, cl = i % kCB, c = c0 + cl;
            if (c >= C || !mrow[(size_t)j * C + c]) continue;
            const int t0 = j * w, l = win_len(j, w, T);
            float sum = 0.f;
            for (int k = 0; k < l; ++k) sum += U[(t0 + k) * kCB + cl];
            const float mean = sum / (float)l;
            for (int k = 0; k < l; ++k) {
                const size_t tc = (size_t)(t0 + k) * C + c;
                const float sd = a.stdv ? a.stdv[tc] : 1.0f;
                a.out[base + tc] += mean / sd;
            }
        }
        return;
    }

    const int lane = tid & 63, wave = tid >> 6, nw = kThreads / 64;
    const int li = lane & 15, kq = lane >> 4;
    const float* Aw = a.p.basis;
    const float* Bw = a.p.basis + (size_t)Jp * Tp;

    // ---- phase 2: R = m . (A_w U) (row i of the tile = window j0 + i)
    for (int tile = wave; tile < Jp / 16; tile += nw) {
        const int j0 = tile * 16;
        const f32x4 acc = tile_product(Aw, j0, Tp, U, li, kq);
        const int c = c0 + li;
        f32x4 r;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int j = j0 + 4 * kq + v;
            const bool keep = j < J && c < C && mrow[(size_t)j * C + c];
            r[v] = keep ? acc[v] : 0.f;
        }
        *reinterpret_cast<f32x4*>(R + ((j0 / 4 + kq) * kCB + li) * 4) = r;
    }
    __syncthreads();

    // ---- phase 3: Y = B_w R (row i of the tile = packed row r0 + i); out += Y / sigma
    for (int tile = wave; tile < Tp / 16; tile += nw) {
        const int r0 = tile * 16;
        const f32x4 acc = tile_product(Bw, r0, Jp, R, li, kq);
        const int c = c0 + li;
        if (c >= C) continue;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int r = r0 + 4 * kq + v;
            if (r >= T) continue;
            const size_t e = base + (size_t)r * C + c;
            const float sd = a.stdv ? a.stdv[(size_t)r * C + c] : 1.0f;
            a.out[e] = a.out[e] + acc[v] / sd;
        }
    }
}

template <bool FOURIER>
__global__ __launch_bounds__(kThreads) void k_dps_residual_agg(fd_agg_res_args a) {
    extern __shared__ float lds[];
    __shared__ double red[kThreads];
    float* U = lds;                            // FOURIER: sigma (x0_obs - x0_hat) / rho, frequency rows (k-quad); else time rows [t][channel]
    float* R = lds + (size_t)a.Tp * kCB;       // FOURIER: r / l, window rows (k-quad)
    const int tid = threadIdx.x;
    const int b = blockIdx.x / a.ncb, c0 = (blockIdx.x % a.ncb) * kCB;
    const int T = a.T, C = a.C, Tp = a.Tp, J = a.p.J, Jp = a.p.Jp, w = a.p.window;
    const size_t TC = (size_t)T * C, base = (size_t)b * TC, obase = (size_t)(b / a.obs_rep) * TC;
    const uint8_t* mrow = a.mask + (a.mask_per_series ? (size_t)(b / a.obs_rep) * J * C : 0);
    double rr = 0.0;

    if (FOURIER) {
        for (int i = tid; i < Tp * kCB; i += kThreads) U[i] = 0.f;
        __syncthreads();
    }
    // ---- phase 1
    for (int i = tid; i < T * kCB; i += kThreads) {
        const int k = i / kCB, cl = i % kCB, c = c0 + cl;
        if (c >= C) continue;
        const size_t kc = (size_t)k * C + c, e = base + kc;
        const float Gk = a.G[k];
        const float sd = a.stdv ? a.stdv[kc] : 1.0f;
        const float x0h = (a.x[e] + a.s2 * (Gk * Gk) * a.score[e]) / a.alpha;
        const float dv = sd * (a.x0[obase + kc] - x0h);
        if (FOURIER) U[quad_idx(k, cl)] = dv * inv_r(k, T);
        else U[i] = dv;
    }
    __syncthreads();

    if (!FOURIER) {
        // ---- one thread per (window, channel): r = the masked mean in ascending t; u = sigma r / l over the window
        for (int i = tid; i < J * kCB; i += kThreads) {
            const int j = i / kCB, cl = i % kCB, c = c0 + cl;
            if (c >= C) continue;
            const int t0 = j * w, l = win_len(j, w, T);
            float r = 0.f;
            if (mrow[(size_t)j * C + c]) {
                float sum = 0.f;
                for (int k = 0; k < l; ++k) sum += U[(t0 + k) * kCB + cl];
                r = sum / (float)l;
            }
            rr += (double)r * (double)r;
            const float rl = r / (float)l;
            for (int k = 0; k < l; ++k) {
                const int t = t0 + k;
                const size_t tc = (size_t)t * C + c, e = base + tc;
                const float sd = a.stdv ? a.stdv[tc] : 1.0f;
                const float uv = sd * rl;
                a.u[e] = uv;
                if (a.dout) {
                    const float Gt = a.G[t];
                    a.dout[e] = a.s2 * (Gt * Gt) * uv;
                }
            }
        }
    } else {
        const int lane = tid & 63, wave = tid >> 6, nw = kThreads / 64;
        const int li = lane & 15, kq = lane >> 4;
        const float* Aw = a.p.basis;
        const float* Bw = a.p.basis + (size_t)Jp * Tp;
        // ---- phase 2: r = m . (A_w U) (row i of the tile = window j0 + i), its squares in double; R = r / l
        for (int tile = wave; tile < Jp / 16; tile += nw) {
            const int j0 = tile * 16;
            const f32x4 acc = tile_product(Aw, j0, Tp, U, li, kq);
            const int c = c0 + li;
            f32x4 r;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int j = j0 + 4 * kq + v;
                const bool keep = j < J && c < C && mrow[(size_t)j * C + c];
                const float rv = keep ? acc[v] : 0.f;
                rr += (double)rv * (double)rv;
                r[v] = keep ? rv / (float)win_len(j, w, T) : 0.f;
            }
            *reinterpret_cast<f32x4*>(R + ((j0 / 4 + kq) * kCB + li) * 4) = r;
        }
        __syncthreads();
        // ---- phase 3: Y = B_w R = F P^T r (row i of the tile = packed row r0 + i); u = sigma Y / rho, dout = s^2 G^2 u
        for (int tile = wave; tile < Tp / 16; tile += nw) {
            const int r0 = tile * 16;
            const f32x4 acc = tile_product(Bw, r0, Jp, R, li, kq);
            const int c = c0 + li;
            if (c >= C) continue;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int k = r0 + 4 * kq + v;
                if (k >= T) continue;
                const size_t kc = (size_t)k * C + c, e = base + kc;
                const float sd = a.stdv ? a.stdv[kc] : 1.0f;
                const float uv = sd * inv_r(k, T) * acc[v];
                a.u[e] = uv;
                if (a.dout) {
                    const float Gk = a.G[k];
                    a.dout[e] = a.s2 * (Gk * Gk) * uv;
                }
            }
        }
    }
    // the block's sum r^2: fixed-order LDS tree
    red[tid] = rr;
    __syncthreads();
#pragma unroll
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) a.part[blockIdx.x] = red[0];
}

// A_w[j][k] = (1 / l_j) sum_{t in window j} F[k][t] and B_w[k][j] = sum_{t in window j} F[k][t] (F of k_impute_basis: packed row k,
// time t), zero outside [0, J) x [0, T); the sums in double in ascending t, then rounded
__global__ __launch_bounds__(256) void k_agg_basis(float* __restrict__ Aw, float* __restrict__ Bw, int T, int Tp, int w, int J, int Jp) {
    const size_t n = (size_t)Jp * Tp;
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int j = (int)(i / Tp), k = (int)(i % Tp);
        double sum = 0.0;
        int l = 1;
        if (j < J && k < T) {
            const int n_real = T / 2 + 1;
            const bool im = k >= n_real;
            const int kk = im ? k - n_real + 1 : k;
            l = win_len(j, w, T);
            for (int t = j * w; t < j * w + l; ++t) {
                double sn, cs;
                sincospi(2.0 * (double)(((long long)kk * t) % T) / (double)T, &sn, &cs);
                sum += im ? -sn : cs;
            }
            sum /= sqrt((double)T);
        }
        Aw[i] = (float)(sum / (double)l);
        Bw[(size_t)k * Jp + j] = (float)sum;
    }
}

size_t lds_bytes(int T, int Tp, int Jp, bool fourier) {
    return (fourier ? (size_t)(Tp + Jp) : (size_t)T) * kCB * sizeof(float);
}

template <bool STEP, bool FOURIER>
int launch_impute(fd_ctx* ctx, const fd_agg_imp_args& a, hipStream_t s) {
    static unsigned long long attr_set = 0;
    if (fd_first_on_device(attr_set, ctx->device))
        FD_HIP(ctx, hipFuncSetAttribute((const void*)k_impute_agg<STEP, FOURIER>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    hipLaunchKernelGGL((k_impute_agg<STEP, FOURIER>), dim3((unsigned)(a.B * a.ncb)), dim3(kThreads),
                       lds_bytes(a.T, a.Tp, a.p.Jp, FOURIER), s, a);
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}

template <bool FOURIER>
int launch_residual(fd_ctx* ctx, const fd_agg_res_args& r, int B, hipStream_t s) {
    static unsigned long long attr_set = 0;
    if (fd_first_on_device(attr_set, ctx->device))
        FD_HIP(ctx, hipFuncSetAttribute((const void*)k_dps_residual_agg<FOURIER>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    hipLaunchKernelGGL((k_dps_residual_agg<FOURIER>), dim3((unsigned)(B * r.ncb)), dim3(kThreads), lds_bytes(r.T, r.Tp, r.p.Jp, FOURIER),
                       s, r);
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}

// ctx->fft_tw key of (T, window), T and window in [1, 1024]: below every key of fd_fourier.hip (T, -T, -T - 2^20) and of
// fd_impute_basis (-T - 2^21)
int basis_key(int T, int window) { return -(3 << 20) - ((window - 1) * 1025 + T); }

const float* agg_basis(fd_ctx* ctx, int T, int Tp, int window, int J, int Jp, hipStream_t s) {
    const int key = basis_key(T, window);
    for (auto& e : ctx->fft_tw)
        if (e.first == key) return reinterpret_cast<const float*>(e.second);
    const size_t n = (size_t)Jp * Tp;
    void* d = nullptr;
    if (hipMalloc(&d, sizeof(float) * 2 * n) != hipSuccess) return nullptr;
    float* Aw = reinterpret_cast<float*>(d);
    hipLaunchKernelGGL(k_agg_basis, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, s, Aw, Aw + n, T, Tp, window, J, Jp);
    // once per (context, T, window): later callers may use another stream
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        (void)hipFree(d);
        return nullptr;
    }
    ctx->fft_tw.emplace_back(key, d);
    return Aw;
}

}  // namespace

int fd_agg_prepare(fd_ctx* ctx, int T, int Tp, int window, int fourier, hipStream_t s, fd_agg_plan* out, const char* who) {
    FD_REQUIRE(ctx, window >= 1 && window <= T, "%s: window=%d must lie in [1, max_len=%d]", who, window, T);
    FD_REQUIRE(ctx, T <= 1024, "%s: max_len %d > 1024 with window > 1 (the LDS images of one series)", who, T);
    out->window = window;
    out->J = (T + window - 1) / window;
    out->Jp = (out->J + 15) / 16 * 16;
    out->basis = nullptr;
    if (fourier) {
        out->basis = agg_basis(ctx, T, Tp, window, out->J, out->Jp, s);
        if (!out->basis) return fd_fail(ctx, FD_ERR_HIP, "%s: could not build the window bases of T=%d window=%d", who, T, window);
    }
    return FD_OK;
}

int fd_agg_launch_impute(fd_ctx* ctx, const fd_agg_imp_args& a, bool step, bool fourier, hipStream_t s) {
    if (step) return fourier ? launch_impute<true, true>(ctx, a, s) : launch_impute<true, false>(ctx, a, s);
    return fourier ? launch_impute<false, true>(ctx, a, s) : launch_impute<false, false>(ctx, a, s);
}

int fd_agg_launch_residual(fd_ctx* ctx, const fd_agg_res_args& r, int B, bool fourier, hipStream_t s) {
    return fourier ? launch_residual<true>(ctx, r, B, s) : launch_residual<false>(ctx, r, B, s);
}
