// fd_impute.hip -- conditional sampling: imputation and forecasting from observed time-domain values (NOT in the reference;
// Song et al. 2021, Sec. 5 and App. I.2, the "inpainter" of score_sde).  After every reverse step the observed coordinates are
// replaced by the observation noised to the next time level.  The observations live in the time domain at data scale, the
// diffusion state in the standardised frequency domain, so the projection is a transform round trip:
//
//   d  = alpha x0_obs + s G z - x                     (sample space; G along T as in fd_perturb)
//   x' = x + dft(m . idft(sigma . d)) / sigma         (fourier = 0: x' = m ? alpha x0_obs + s G z : x)
//
// which is A^-1(m . A(x_obs) + (1 - m) . A(x)) with A(x) = idft(sigma . x + mu): mu cancels, and so does the value of y at
// unobserved entries.
//
// The packed real DFT as a T x T matrix F (y = F x, rows [0, T/2] Re X_k, rows (T/2, T) Im X_k, ortho norm) has orthogonal rows,
// F F^T = diag(r) with r = 1 at DC and Nyquist (T even) and 1/2 elsewhere, so idft = F^T diag(1/r): one basis per T serves both
// directions.  It is built once on the device in double, rounded to f32, zero-padded to Tp = 16 ceil(T/16) and cached on the
// context next to the FFT tables (F and F^T, both row-major, so that both products read 16-byte runs along their k axis).
//
// One workgroup per (series, block of 16 channels).  Phase 1 (elementwise, Philox groups of 4 elements as k_sde_step): the
// reverse-SDE step (fd_sde_apply, the expression of k_sde_step), then d; x_new goes to `out`, sigma d / r to the LDS image U.
// Phase 2: V = F^T U (v_mfma_f32_16x16x4_f32, 16 time rows x 16 channels per tile), masked into the LDS image W.  Phase 3:
// Y = F W, out += Y / sigma.  Both LDS images are Tp x 16 floats in k-quad order, [(k / 4)][channel][k % 4], so that the
// B operand of four consecutive MFMAs is one conflict-free ds_read_b128 per lane; LDS = 128 Tp bytes (128 KiB at T = 1024).
// The images, the product, the group walk of phase 1 and the launch are fd_project.h's, shared with k_dps_residual (fd_dps.hip).
//
// The mask enters in one place, between the two products, so k_impute is a template on the observation operator (fd_project.h):
// MaskOp is the above; WindowOp conditions on window means (fd_aggregate.hip: the middle image holds windows, the bases are
// A_w / B_w) and adds the one body that differs, the time-domain window sum; DenseOp conditions on a matrix the caller supplies
// (fd_linop.hip: the middle image holds its rows, the bases are the operator's own) and runs the two products in both domains.
//
// RePaint resampling (Lugmayr et al. 2022; fd_sampler_run_impute_repaint): the steps are cut into blocks of jump_length, each block
// runs `resample` times, and between two runs the state is diffused forward from the block's last level to its first by the
// transition kernel, x <- ra x + rb G z_r.  The projector P = A^-1 m A is linear, so
//   ra (x_s + P(x_obs - x_s)) + rb G z_r = xt + P(ra d),   xt = ra x_s + rb G z_r,
// and the re-noise folds into phase 1 of the block's last step (RENOISE): one more Philox group, xt to `out`, ra sigma d / r to U.
#include <algorithm>
#include <cmath>
#include <vector>

#include "fd_aggregate.h"
#include "fd_common.h"
#include "fd_engine.h"
#include "fd_linop.h"
#include "fd_loop.h"
#include "fd_project.h"
#include "fd_sde.h"

namespace {

using namespace fdproj;

struct ImpArgs {
    const float* x;          // (B,T,C) state before the step (may alias out)
    const float* score;      // (B,T,C) score at t_i (STEP only)
    const float* zstep;      // (B,T,C) injected predictor noise or nullptr (Philox at off_step)
    const float* x0;         // (B/obs_rep,T,C) A^-1(where(m, y, 0)): state row b reads observation row b / obs_rep
    const uint8_t* mask;     // (B/obs_rep,M,C) or (M,C), 1 = observed, over the operator's M rows (time steps / windows)
    const float* stdv;       // (T,C) feature std of the packed spectrum or nullptr (= 1)
    const float* G;          // (T)
    const float* zobs;       // (B,T,C) injected observation noise or nullptr (Philox at off_obs)
    const float* basis;      // the operator's pair: F then F^T (Tp x Tp each), or A_w (Jp x Tp) then B_w (Tp x Jp); the dense
                             // operator carries its own
    float* out;
    int B, T, C, Tp, ncb, mask_per_series, obs_rep;
    SdeCoef cf;
    float alpha, s;
    uint64_t seed, off_step, off_obs;
    // RENOISE only
    const float* zre;        // (B,T,C) injected re-noise or nullptr (Philox at off_re)
    float ra, rb;            // the forward transition kernel between the two levels: x <- ra x + rb G z_r
    uint64_t off_re;
};
// PAIR (classifier-free guidance, fd_loop.h): x, score and out are (2B,T,C), rows [B, 2B) the null-token twin of rows [0, B)
struct ImpArgsPair : ImpArgs {
    float w, omw;            // the guidance scale and 1 - w
};
template <bool PAIR>
struct ImpArgsOf { typedef ImpArgs type; };
template <>
struct ImpArgsOf<true> { typedef ImpArgsPair type; };

// Op (fd_project.h): the coordinate mask, or window means (fd_aggregate.hip) or a dense operator (fd_linop.hip), which go with
// neither PAIR nor RENOISE.
// PAIR: the workgroup of (b, channel block) reads x[b], steps with the guided score fd_guided(score[b], score[B + b]) and writes
// every final value to rows b and B + b, so the two halves stay bit-equal; the Philox counters and lanes are those of the unpaired
// launch over n = B T C (the second half draws nothing).
// RENOISE: the projected state is diffused forward in the same pass, out = ra (projected x) + rb G z_r (see the head of the file).
template <bool STEP, bool FOURIER, bool PAIR, bool RENOISE, class Op>
__global__ __launch_bounds__(kThreads) void k_impute(typename ImpArgsOf<PAIR>::type a, Op op) {
    static_assert(!(Op::kWindow && (PAIR || RENOISE)), "window means go with neither a guide nor RePaint");
    static_assert(!(Op::kDense && (PAIR || RENOISE)), "a dense operator goes with neither a guide nor RePaint");
    constexpr bool IMAGE = FOURIER || Op::kWindow || Op::kDense;      // the mask in the time domain selects elementwise: no LDS
    constexpr bool PRODUCTS = FOURIER || Op::kDense;    // the two MFMA products: a dense operator in the time domain is the Fourier
                                                        // branch with rho = 1 on the time-domain bases
    extern __shared__ float lds[];
    float* U = lds;                            // PRODUCTS: sigma d / r, packed rows (k-quad); else sigma d, time rows [t][channel]
    float* W = lds + (size_t)a.Tp * kCB;       // PRODUCTS: m . (the observed rows of idft(sigma d)), the operator's rows (k-quad)
    const int tid = threadIdx.x;
    const int b = blockIdx.x / a.ncb, c0 = (blockIdx.x % a.ncb) * kCB;
    const int T = a.T, C = a.C, Tp = a.Tp, M = op.rows(T), Mp = op.rows_padded(Tp);
    const size_t TC = (size_t)T * C, base = (size_t)b * TC, obase = (size_t)(b / a.obs_rep) * TC;
    const uint8_t* mrow = a.mask + (a.mask_per_series ? (size_t)(b / a.obs_rep) * M * C : 0);
    [[maybe_unused]] const size_t half = (size_t)a.B * TC;      // PAIR: the null half of x / score / out starts here

    if (PRODUCTS) {
        for (int i = tid; i < Tp * kCB; i += kThreads) U[i] = 0.f;
        __syncthreads();
    }

    // ---- phase 1: step + d, over the Philox groups that touch this series
    const size_t g_lo = base / 4, g_hi = (base + TC + 3) / 4;
    for (size_t g = g_lo + tid; g < g_hi; g += kThreads) {
        int loc[4];
        bool own[4];
        if (!group_of(g, base, TC, C, c0, loc, own)) continue;
        float zs[4] = {0.f, 0.f, 0.f, 0.f}, zo[4] = {0.f, 0.f, 0.f, 0.f};
        [[maybe_unused]] float zr[4] = {0.f, 0.f, 0.f, 0.f};
        if (STEP) group_noise(loc, own, a.zstep, base, a.off_step + g, a.seed, zs);
        if (a.s != 0.f) group_noise(loc, own, a.zobs, base, a.off_obs + g, a.seed, zo);      // the hard projection (s = 0) reads none
        if constexpr (RENOISE) group_noise(loc, own, a.zre, base, a.off_re + g, a.seed, zr);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!own[j]) continue;
            const size_t e = base + loc[j];
            const int t = loc[j] / C, c = loc[j] % C;
            const float Gt = a.G[t];
            float xv = a.x[e];
            if (STEP) {
                float sc = a.score[e];
                if constexpr (PAIR) sc = fd_guided(sc, a.score[half + e], a.w, a.omw);
                xv = fd_sde_apply(xv, sc, zs[j], Gt, a.cf);
            }
            const float xo = a.alpha * a.x0[obase + loc[j]] + a.s * (Gt * zo[j]);
            if constexpr (!IMAGE) {
                float o = mrow[(size_t)t * C + c] ? xo : xv;
                if constexpr (RENOISE) {       // (both sums written out: selecting first contracts differently and moves the last bit)
                    const float nz = a.rb * (Gt * zr[j]);
                    o = mrow[(size_t)t * C + c] ? a.ra * xo + nz : a.ra * xv + nz;
                }
                a.out[e] = o;
                if constexpr (PAIR) a.out[half + e] = o;
            } else {
                float xt = xv, dv = xo - xv;       // what goes to `out` before the projection, and d
                if constexpr (RENOISE) {
                    xt = a.ra * xv + a.rb * (Gt * zr[j]);
                    dv = a.ra * dv;
                }
                a.out[e] = xt;
                const float sd = a.stdv ? a.stdv[(size_t)t * C + c] : 1.0f;
                if (FOURIER) U[quad_idx(t, c - c0)] = sd * dv * inv_r(t, T);
                else if (Op::kDense) U[quad_idx(t, c - c0)] = sd * dv;
                else U[t * kCB + (c - c0)] = sd * dv;
            }
        }
    }
    if constexpr (IMAGE) __syncthreads();     // U complete; out holds x_new (workgroup-scope release / acquire covers the global stores)

    if constexpr (Op::kWindow && !FOURIER) {
        // ---- window means in the time domain: one thread per (window, channel), the mean in ascending t, masked, written back
        // over the window
        for (int i = tid; i < M * kCB; i += kThreads) {
            const int j = i / kCB, cl = i % kCB, c = c0 + cl;
            if (c >= C || !mrow[(size_t)j * C + c]) continue;
            const int t0 = j * op.window, l = win_len(j, op.window, T);
            float sum = 0.f;
            for (int k = 0; k < l; ++k) sum += U[(t0 + k) * kCB + cl];
            const float mean = sum / (float)l;
            for (int k = 0; k < l; ++k) {
                const size_t tc = (size_t)(t0 + k) * C + c;
                const float sd = a.stdv ? a.stdv[tc] : 1.0f;
                a.out[base + tc] += mean / sd;
            }
        }
    }
    if constexpr (FOURIER || Op::kDense) {
        const int lane = tid & 63, wave = tid >> 6, nw = kThreads / 64;
        const int li = lane & 15, kq = lane >> 4;
        const int c = c0 + li;
        const float* Ao = op.to_obs(a.basis, Tp);
        const float* Bo = op.from_obs(a.basis, Tp);

        // ---- phase 2: W = m . (Ao U) (row i of the tile = observation row j0 + i: a time step or a window)
        for (int tile = wave; tile < Mp / 16; tile += nw) {
            const int j0 = tile * 16;
            const f32x4 acc = tile_product(Ao, j0, Tp, U, li, kq);
            f32x4 w;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int j = j0 + 4 * kq + v;
                const bool keep = j < M && c < C && mrow[(size_t)j * C + c];
                w[v] = keep ? acc[v] : 0.f;
            }
            *reinterpret_cast<f32x4*>(W + ((j0 / 4 + kq) * kCB + li) * 4) = w;
        }
        __syncthreads();

        // ---- phase 3: Y = Bo W (row i of the tile = packed row r0 + i); out += Y / sigma
        for (int tile = wave; tile < Tp / 16; tile += nw) {
            const int r0 = tile * 16;
            const f32x4 acc = tile_product(Bo, r0, Mp, W, li, kq);
            if (c >= C) continue;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int r = r0 + 4 * kq + v;
                if (r >= T) continue;
                const size_t e = base + (size_t)r * C + c;
                const float sd = a.stdv ? a.stdv[(size_t)r * C + c] : 1.0f;
                const float o = a.out[e] + acc[v] / sd;
                a.out[e] = o;
                if constexpr (PAIR) a.out[half + e] = o;
            }
        }
    }
}

// F[r][t] (packed row r, time t) and its transpose, zero outside [0, T)^2, in double then rounded
__global__ __launch_bounds__(256) void k_impute_basis(float* __restrict__ Fm, float* __restrict__ Ft, int T, int Tp) {
    const size_t n = (size_t)Tp * Tp;
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int r = (int)(i / Tp), t = (int)(i % Tp);
        float v = 0.f;
        if (r < T && t < T) {
            const int n_real = T / 2 + 1;
            const bool im = r >= n_real;
            const int k = im ? r - n_real + 1 : r;
            double sn, cs;
            sincospi(2.0 * (double)(((long long)k * t) % T) / (double)T, &sn, &cs);
            v = (float)((im ? -sn : cs) / sqrt((double)T));
        }
        Fm[i] = v;
        Ft[(size_t)t * Tp + r] = v;
    }
}

template <bool STEP, bool FOURIER, bool PAIR = false, bool RENOISE = false, class Op = MaskOp>
int launch_variant(fd_ctx* ctx, const typename ImpArgsOf<PAIR>::type& a, hipStream_t s, Op op = Op()) {
    return launch_kernel<k_impute<STEP, FOURIER, PAIR, RENOISE, Op>, (Op::kWindow || Op::kDense ? 128 : 160) * 1024>(
        ctx, (unsigned)(a.B * a.ncb), image_bytes(op, a.T, a.Tp, FOURIER), s, a, op);
}

// fills the shape / conditioning fields of `a` and checks them
int prepare(fd_ctx* ctx, ImpArgs& a, const float* x0, const uint8_t* mask, int mask_per_series, const float* stdv, int fourier,
            const float* G, int B, int T, int C, hipStream_t s, const char* who) {
    FD_REQUIRE(ctx, x0 && mask && G, "%s: null pointer", who);
    FD_REQUIRE(ctx, B > 0 && T > 0 && C > 0, "%s: B=%d T=%d C=%d", who, B, T, C);
    FD_REQUIRE(ctx, !fourier || T <= 1024, "%s: max_len %d > 1024 (the LDS images of one series)", who, T);
    a.B = B; a.T = T; a.C = C;
    a.Tp = (T + 15) / 16 * 16;
    a.ncb = (C + kCB - 1) / kCB;
    FD_REQUIRE(ctx, (long long)B * a.ncb < (1ll << 31), "%s: B=%d too large for one launch", who, B);
    a.x0 = x0; a.mask = mask; a.mask_per_series = mask_per_series ? 1 : 0;
    a.obs_rep = 1;
    a.stdv = fourier ? stdv : nullptr;
    a.G = G;
    a.basis = nullptr;
    if (fourier) {
        a.basis = fd_impute_basis(ctx, T, a.Tp, s);
        if (!a.basis) return fd_fail(ctx, FD_ERR_HIP, "%s: could not build the transform basis of T=%d", who, T);
    }
    return FD_OK;
}

// renoise (the mask alone): the RENOISE variants (a.ra, a.rb, a.zre, a.off_re set): the loop's fused step, or the step-wise projection
template <class Op = MaskOp>
int launch(fd_ctx* ctx, const ImpArgs& a, bool step, bool fourier, hipStream_t s, bool renoise = false, Op op = Op()) {
    if constexpr (!Op::kWindow && !Op::kDense)
        if (renoise) {
            if (step) return fourier ? launch_variant<true, true, false, true>(ctx, a, s) : launch_variant<true, false, false, true>(ctx, a, s);
            return fourier ? launch_variant<false, true, false, true>(ctx, a, s) : launch_variant<false, false, false, true>(ctx, a, s);
        }
    if (step)
        return fourier ? launch_variant<true, true, false, false>(ctx, a, s, op) : launch_variant<true, false, false, false>(ctx, a, s, op);
    return fourier ? launch_variant<false, true, false, false>(ctx, a, s, op) : launch_variant<false, false, false, false>(ctx, a, s, op);
}

// the guided step + projection on the paired state (a.B series, 2 a.B rows)
int launch_pair(fd_ctx* ctx, const ImpArgs& a, const fd_guide& g, bool fourier, hipStream_t s, bool renoise = false) {
    ImpArgsPair ap{};
    static_cast<ImpArgs&>(ap) = a;
    ap.w = g.w;
    ap.omw = g.omw;
    if (renoise) return fourier ? launch_variant<true, true, true, true>(ctx, ap, s) : launch_variant<true, false, true, true>(ctx, ap, s);
    return fourier ? launch_variant<true, true, true>(ctx, ap, s) : launch_variant<true, false, true>(ctx, ap, s);
}

// window means: the geometry of (T, window) and, in `a`, what the window operator reads in the mask's place (fd_aggregate.h)
int prepare_window(fd_ctx* ctx, ImpArgs& a, int window, const float* stdv, int fourier, hipStream_t s, fd_agg_plan* agg, const char* who) {
    if (int rc = fd_agg_prepare(ctx, a.T, a.Tp, window, fourier, s, agg, who)) return rc;
    a.stdv = stdv;
    a.basis = agg->basis;
    return FD_OK;
}

// a dense operator: its bases in the call's domain and, in `a`, the feature std, which both domains read (fd_linop.h)
int prepare_dense(fd_ctx* ctx, ImpArgs& a, fd_linop* lop, const float* stdv, int fourier, hipStream_t s, DenseOp* dop, const char* who) {
    if (int rc = fd_linop_prepare(ctx, lop, a.T, fourier, s, dop, who)) return rc;
    a.stdv = stdv;
    return FD_OK;
}

// (alpha, s) of level i of an n-step grid: the perturbation kernel at timesteps[i], the clean level (1, 0) at i = n
void level_coef(const fd_sde_params& sde, const float* timesteps, int n_steps, int i, double* alpha, double* sdev) {
    *alpha = 1.0;
    *sdev = 0.0;
    if (i < n_steps) fd_marginal_coef(sde, (double)timesteps[i], alpha, sdev);
}

// The loop behind fd_sampler_run_impute_rep (g == null), fd_sampler_run_impute_cfg and fd_sampler_run_impute_repaint: the arguments of
// the first, checked under the name `who`; a paired guide runs on x (2B,T,C) with its labels (2B) behind the score.  resample = r,
// jump_length = j: the steps are cut into blocks [i0, min(i0 + j, n_steps)), each block runs r times, and the last step of every run
// but the r-th re-noises from level i1 back to level i0 (RENOISE); r = 1 is the plain loop for every j.  E = r n_steps evaluations, K =
// (r - 1) ceil(n_steps / j) re-noises; z_steps, zobs_steps (E,B,T,C) and zre_steps (K,B,T,C) in execution order.  window > 1 or lop
// (not both): the mask holds the operator's rows.
int impute_loop(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps, float dt, float* x,
                const float* x0_obs, const uint8_t* mask_u8, int mask_per_series, const float* feat_std, int fourier,
                const float* z_steps, const float* zobs_steps, uint64_t seed, uint64_t offset, int B, int obs_replicas, int mode,
                hipStream_t s, const fd_guide* g, const char* who, const float* zre_steps = nullptr, int resample = 1,
                int jump_length = 1, int window = 1, fd_linop* lop = nullptr) {
    fd_ctx* ctx = m->ctx;
    FD_REQUIRE(ctx, G && timesteps && x, "%s: null pointer", who);
    FD_REQUIRE(ctx, n_steps > 0, "%s: n_steps=%d", who, n_steps);
    FD_REQUIRE(ctx, dt > 0.f, "%s: step size must be > 0 (sde.py:158)", who);
    FD_REQUIRE(ctx, obs_replicas > 0 && B % obs_replicas == 0, "%s: B=%d is not a multiple of obs_replicas=%d", who, B, obs_replicas);
    FD_REQUIRE(ctx, resample >= 1 && jump_length >= 1, "%s: resample=%d jump_length=%d must be >= 1", who, resample, jump_length);
    FD_REQUIRE(ctx, (long long)resample * n_steps < (1ll << 31), "%s: resample=%d x n_steps=%d evaluations", who, resample, n_steps);
    const int T = m->d.max_len, C = m->d.n_channels;
    ImpArgs a{};
    if (int rc = prepare(ctx, a, x0_obs, mask_u8, mask_per_series, feat_std, fourier, G, B, T, C, s, who)) return rc;
    a.obs_rep = obs_replicas;
    // window > 1: the mask holds windows and k_impute runs on the window operator (no guide and no RePaint there)
    fd_agg_plan agg{};
    if (window > 1) {
        FD_REQUIRE(ctx, !g && resample == 1, "%s: window=%d goes with neither a guide nor resample > 1", who, window);
        if (int rc = prepare_window(ctx, a, window, feat_std, fourier, s, &agg, who)) return rc;
    }
    DenseOp dop{};
    if (lop) {
        FD_REQUIRE(ctx, !g && resample == 1 && window == 1, "%s: an operator goes with no guide, resample > 1 or window > 1", who);
        if (int rc = prepare_dense(ctx, a, lop, feat_std, fourier, s, &dop, who)) return rc;
    }
    // per-step coefficients, on the host up front: the SDE step's (fd_sde_coef, as fd_sampler_run) and the projection's (alpha, s)
    // at the next grid point; the last step projects hard (alpha = 1, s = 0)
    std::vector<SdeCoef> cf(n_steps);
    std::vector<float> al(n_steps), sd(n_steps);
    for (int i = 0; i < n_steps; ++i) {
        cf[i] = fd_sde_coef(*sde, (double)timesteps[i], dt);
        double aa, ss;
        level_coef(*sde, timesteps, n_steps, i + 1, &aa, &ss);
        al[i] = (float)aa;
        sd[i] = (float)ss;
    }
    // the executed steps in order (the evaluation-time table follows them), and the transition kernel of every block, in double:
    // ra = alpha(i0) / alpha(i1), rb^2 = s(i0)^2 - ra^2 s(i1)^2 (the variance the forward process adds between the two levels)
    const int E = resample * n_steps;
    std::vector<int> step_of(E);
    std::vector<float> te(E), ra((size_t)n_steps, 1.f), rb((size_t)n_steps, 0.f);      // ra, rb indexed by the block's last step
    for (int i0 = 0, e = 0; i0 < n_steps; i0 += jump_length) {
        const int i1 = std::min(i0 + jump_length, n_steps);
        for (int r = 0; r < resample; ++r)
            for (int i = i0; i < i1; ++i, ++e) {
                step_of[e] = i;
                te[e] = timesteps[i];
            }
        if (resample > 1) {
            double a0, s0, a1, s1;
            level_coef(*sde, timesteps, n_steps, i0, &a0, &s0);
            level_coef(*sde, timesteps, n_steps, i1, &a1, &s1);
            const double q = a0 / a1, rad = s0 * s0 - q * q * s1 * s1;
            FD_REQUIRE(ctx, rad >= -1e-12, "%s: levels %d -> %d: the transition variance %g is negative (timesteps must decrease)", who,
                       i1, i0, rad);
            ra[i1 - 1] = (float)q;
            rb[i1 - 1] = (float)std::sqrt(std::max(rad, 0.0));
        }
    }
    const size_t n = (size_t)B * T * C;
    const int R = fd_guide_rows(g, B);
    const bool pair = g && g->pair;
    fd_step_loop lp;
    if (int rc = fd_step_loop_open(&lp, m, R, mode, fd_guide_bytes(g, B), te.data(), E, s)) return rc;
    int* lab = (int*)lp.own;
    if (int rc = fd_guide_begin(m, g, lab, x, B, s)) return rc;
    fd_guide_scope scope(m, g, lab, R);

    // Philox counters: predictor noise of executed step e at offset + e*per_step (as fd_sampler_run), observation noise behind them
    // at offset + (E + e)*per_step, re-noise k behind those at offset + (2E + k)*per_step
    const uint64_t per_step = (uint64_t)((n + 3) / 4);
    a.x = x; a.out = x; a.score = lp.score;
    a.seed = seed;
    for (int e = 0, k = 0; e < E; ++e) {
        const int i = step_of[e];
        // the last step of a block's run, unless the run is the block's last: e + 1 then restarts the block
        const bool renoise = e + 1 < E && step_of[e + 1] <= i;
        if (int rc = fd_step_loop_eval(&lp, e, x)) return rc;
        a.zstep = z_steps ? z_steps + (size_t)e * n : nullptr;
        a.zobs = zobs_steps ? zobs_steps + (size_t)e * n : nullptr;
        a.cf = cf[i];
        a.alpha = al[i];
        a.s = sd[i];
        a.off_step = offset + (uint64_t)e * per_step;
        a.off_obs = offset + (uint64_t)(E + e) * per_step;
        if (renoise) {
            a.zre = zre_steps ? zre_steps + (size_t)k * n : nullptr;
            a.ra = ra[i];
            a.rb = rb[i];
            a.off_re = offset + ((uint64_t)2 * E + (uint64_t)k) * per_step;
            ++k;
        }
        if (window > 1) {
            if (int rc = launch(ctx, a, true, fourier != 0, s, false, agg.op)) return rc;
            continue;
        }
        if (lop) {
            if (int rc = launch(ctx, a, true, fourier != 0, s, false, dop)) return rc;
            continue;
        }
        if (int rc = pair ? launch_pair(ctx, a, *g, fourier != 0, s, renoise) : launch(ctx, a, true, fourier != 0, s, renoise)) return rc;
    }
    return FD_OK;
}

}  // namespace

const float* fd_impute_basis(fd_ctx* ctx, int T, int Tp, hipStream_t s) {
    const size_t n = (size_t)Tp * Tp;
    return fdproj::cached_table(ctx, -T - (2 << 20), 2 * n, s, [&](float* Fm) {
        hipLaunchKernelGGL(k_impute_basis, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, s, Fm, Fm + n, T, Tp);
    });
}

// marginal mean coefficient and std of the perturbation kernel at t (sde.py:108-123, 187-210), in double
void fd_marginal_coef(const fd_sde_params& p, double t, double* alpha, double* sdev) {
    if (p.kind == 0) {
        const double lmc = -0.25 * t * t * ((double)p.p1 - (double)p.p0) - 0.5 * t * (double)p.p0;
        *alpha = std::exp(lmc);
        *sdev = std::sqrt(1.0 - std::exp(2.0 * lmc));
    } else {
        *alpha = 1.0;
        *sdev = (double)p.p0 * std::pow((double)p.p1 / (double)p.p0, t);
    }
}

extern "C" int fd_impute_project(fd_ctx* ctx, const float* x, const float* x0_obs, const uint8_t* mask_u8, int mask_per_series,
                                 const float* feat_std, int fourier, const float* G, float alpha, float s, const float* z,
                                 uint64_t seed, uint64_t offset, float* out, int B, int T, int C, void* stream) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, x && out, "fd_impute_project: null pointer");
    hipStream_t hs = (hipStream_t)stream;
    ImpArgs a{};
    if (int rc = prepare(ctx, a, x0_obs, mask_u8, mask_per_series, feat_std, fourier, G, B, T, C, hs, "fd_impute_project")) return rc;
    a.x = x; a.out = out;
    a.zobs = z;
    a.alpha = alpha; a.s = s;
    a.seed = seed; a.off_obs = offset;
    return launch(ctx, a, false, fourier != 0, hs);
}

extern "C" int fd_impute_project_agg(fd_ctx* ctx, const float* x, const float* x0_obs, const uint8_t* mask_u8, int mask_per_series,
                                     const float* feat_std, int fourier, const float* G, float alpha, float s, const float* z,
                                     uint64_t seed, uint64_t offset, float* out, int B, int T, int C, int window, void* stream) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, window >= 1 && window <= T, "fd_impute_project_agg: window=%d must lie in [1, T=%d]", window, T);
    if (window == 1)
        return fd_impute_project(ctx, x, x0_obs, mask_u8, mask_per_series, feat_std, fourier, G, alpha, s, z, seed, offset, out, B, T, C,
                                 stream);
    FD_REQUIRE(ctx, x && out, "fd_impute_project_agg: null pointer");
    hipStream_t hs = (hipStream_t)stream;
    ImpArgs a{};
    if (int rc = prepare(ctx, a, x0_obs, mask_u8, mask_per_series, feat_std, fourier, G, B, T, C, hs, "fd_impute_project_agg")) return rc;
    fd_agg_plan agg{};
    if (int rc = prepare_window(ctx, a, window, feat_std, fourier, hs, &agg, "fd_impute_project_agg")) return rc;
    a.x = x; a.out = out;
    a.zobs = z;
    a.alpha = alpha; a.s = s;
    a.seed = seed; a.off_obs = offset;
    return launch(ctx, a, false, fourier != 0, hs, false, agg.op);
}

extern "C" int fd_impute_project_op(fd_ctx* ctx, const float* x, const float* x0_obs, const uint8_t* mask_u8, int mask_per_series,
                                    const float* feat_std, int fourier, const float* G, float alpha, float s, const float* z,
                                    uint64_t seed, uint64_t offset, float* out, int B, int T, int C, fd_linop* op, void* stream) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, x && out, "fd_impute_project_op: null pointer");
    hipStream_t hs = (hipStream_t)stream;
    ImpArgs a{};
    if (int rc = prepare(ctx, a, x0_obs, mask_u8, mask_per_series, feat_std, 0, G, B, T, C, hs, "fd_impute_project_op")) return rc;
    DenseOp dop{};
    if (int rc = prepare_dense(ctx, a, op, feat_std, fourier, hs, &dop, "fd_impute_project_op")) return rc;
    a.x = x; a.out = out;
    a.zobs = z;
    a.alpha = alpha; a.s = s;
    a.seed = seed; a.off_obs = offset;
    return launch(ctx, a, false, fourier != 0, hs, false, dop);
}

extern "C" int fd_impute_project_renoise(fd_ctx* ctx, const float* x, const float* x0_obs, const uint8_t* mask_u8, int mask_per_series,
                                         const float* feat_std, int fourier, const float* G, float alpha, float s, const float* z,
                                         uint64_t seed, uint64_t offset, float a, float b, const float* z_re, uint64_t offset_re,
                                         float* out, int B, int T, int C, void* stream) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, x && out, "fd_impute_project_renoise: null pointer");
    FD_REQUIRE(ctx, std::isfinite(a) && std::isfinite(b) && b >= 0.f, "fd_impute_project_renoise: a=%g b=%g (finite, b >= 0)", (double)a,
               (double)b);
    hipStream_t hs = (hipStream_t)stream;
    ImpArgs ia{};
    if (int rc = prepare(ctx, ia, x0_obs, mask_u8, mask_per_series, feat_std, fourier, G, B, T, C, hs, "fd_impute_project_renoise"))
        return rc;
    ia.x = x; ia.out = out;
    ia.zobs = z;
    ia.alpha = alpha; ia.s = s;
    ia.seed = seed; ia.off_obs = offset;
    ia.zre = z_re;
    ia.ra = a; ia.rb = b;
    ia.off_re = offset_re;
    return launch(ctx, ia, false, fourier != 0, hs, true);
}

extern "C" int fd_sampler_run_impute_rep(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps,
                                         int n_steps, float dt, float* x, const float* x0_obs, const uint8_t* mask_u8,
                                         int mask_per_series, const float* feat_std, int fourier, const float* z_steps,
                                         const float* zobs_steps, uint64_t seed, uint64_t offset, int B, int obs_replicas, int mode,
                                         void* stream) {
    if (int rc = fd_loop_check(m, sde, B, mode, "fd_sampler_run_impute")) return rc;
    return impute_loop(m, sde, G, timesteps, n_steps, dt, x, x0_obs, mask_u8, mask_per_series, feat_std, fourier, z_steps, zobs_steps,
                       seed, offset, B, obs_replicas, mode, (hipStream_t)stream, nullptr, "fd_sampler_run_impute");
}

// fd_sampler_run_impute_rep on window means: mask_u8 (B/obs_replicas,J,C) or (J,C), J = ceil(T / window); window = 1 is that call
extern "C" int fd_sampler_run_impute_agg(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps,
                                         int n_steps, float dt, float* x, const float* x0_obs, const uint8_t* mask_u8,
                                         int mask_per_series, const float* feat_std, int fourier, const float* z_steps,
                                         const float* zobs_steps, uint64_t seed, uint64_t offset, int B, int obs_replicas, int window,
                                         int mode, void* stream) {
    if (int rc = fd_loop_check(m, sde, B, mode, "fd_sampler_run_impute_agg")) return rc;
    FD_REQUIRE(m->ctx, window >= 1 && window <= m->d.max_len, "fd_sampler_run_impute_agg: window=%d must lie in [1, max_len=%d]", window,
               m->d.max_len);
    if (window == 1)
        return fd_sampler_run_impute_rep(m, sde, G, timesteps, n_steps, dt, x, x0_obs, mask_u8, mask_per_series, feat_std, fourier,
                                         z_steps, zobs_steps, seed, offset, B, obs_replicas, mode, stream);
    return impute_loop(m, sde, G, timesteps, n_steps, dt, x, x0_obs, mask_u8, mask_per_series, feat_std, fourier, z_steps, zobs_steps,
                       seed, offset, B, obs_replicas, mode, (hipStream_t)stream, nullptr, "fd_sampler_run_impute_agg", nullptr, 1, 1,
                       window);
}

// fd_sampler_run_impute_rep on a dense operator: mask_u8 (B/obs_replicas,M,C) or (M,C) over the M rows of `op`
extern "C" int fd_sampler_run_impute_op(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps,
                                        int n_steps, float dt, float* x, const float* x0_obs, const uint8_t* mask_u8,
                                        int mask_per_series, const float* feat_std, int fourier, const float* z_steps,
                                        const float* zobs_steps, uint64_t seed, uint64_t offset, int B, int obs_replicas, fd_linop* op,
                                        int mode, void* stream) {
    if (int rc = fd_loop_check(m, sde, B, mode, "fd_sampler_run_impute_op")) return rc;
    FD_REQUIRE(m->ctx, op, "fd_sampler_run_impute_op: null operator handle");
    return impute_loop(m, sde, G, timesteps, n_steps, dt, x, x0_obs, mask_u8, mask_per_series, feat_std, fourier, z_steps, zobs_steps,
                       seed, offset, B, obs_replicas, mode, (hipStream_t)stream, nullptr, "fd_sampler_run_impute_op", nullptr, 1, 1, 1,
                       op);
}

// fd_sampler_run_impute_rep on a class-conditional model under classifier-free guidance: y (B) one label per state row or null,
// w the guidance scale.  Labels and w outside {0, 1} (or FDIFF_CFG_FORCE_PAIR): x is (2B,T,C) with the state in its first half, the
// two evaluations of a step run as one forward on 2B rows and k_impute<.., PAIR> steps and projects on the guided score; else one
// evaluation on B rows with y bound (w = 0 or y null: the null token), the unpaired kernel.
extern "C" int fd_sampler_run_impute_cfg(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps,
                                         int n_steps, float dt, float* x, const float* x0_obs, const uint8_t* mask_u8,
                                         int mask_per_series, const float* feat_std, int fourier, const float* z_steps,
                                         const float* zobs_steps, uint64_t seed, uint64_t offset, int B, int obs_replicas, int mode,
                                         const int32_t* y, float cfg_scale, void* stream) {
    if (int rc = fd_loop_check(m, sde, B, mode, "fd_sampler_run_impute_cfg")) return rc;
    if (int rc = fd_guide_check(m, cfg_scale, "fd_sampler_run_impute_cfg")) return rc;
    const fd_guide g = fd_guide_plan(y, cfg_scale);
    return impute_loop(m, sde, G, timesteps, n_steps, dt, x, x0_obs, mask_u8, mask_per_series, feat_std, fourier, z_steps, zobs_steps,
                       seed, offset, B, obs_replicas, mode, (hipStream_t)stream, &g, "fd_sampler_run_impute_cfg");
}

// fd_sampler_run_impute_cfg with RePaint resampling (see impute_loop); y null and cfg_scale = 1: the unguided loop, on any model
extern "C" int fd_sampler_run_impute_repaint(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps,
                                             int n_steps, float dt, float* x, const float* x0_obs, const uint8_t* mask_u8,
                                             int mask_per_series, const float* feat_std, int fourier, const float* z_steps,
                                             const float* zobs_steps, uint64_t seed, uint64_t offset, int B, int obs_replicas, int mode,
                                             const int32_t* y, float cfg_scale, const float* zre_steps, int resample, int jump_length,
                                             void* stream) {
    const char* who = "fd_sampler_run_impute_repaint";
    if (int rc = fd_loop_check(m, sde, B, mode, who)) return rc;
    const bool guided = y || cfg_scale != 1.0f;
    fd_guide g{};
    if (guided) {
        if (int rc = fd_guide_check(m, cfg_scale, who)) return rc;
        g = fd_guide_plan(y, cfg_scale);
    }
    return impute_loop(m, sde, G, timesteps, n_steps, dt, x, x0_obs, mask_u8, mask_per_series, feat_std, fourier, z_steps, zobs_steps,
                       seed, offset, B, obs_replicas, mode, (hipStream_t)stream, guided ? &g : nullptr, who, zre_steps, resample,
                       jump_length);
}

extern "C" int fd_sampler_run_impute(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps,
                                     float dt, float* x, const float* x0_obs, const uint8_t* mask_u8, int mask_per_series,
                                     const float* feat_std, int fourier, const float* z_steps, const float* zobs_steps,
                                     uint64_t seed, uint64_t offset, int B, int mode, void* stream) {
    return fd_sampler_run_impute_rep(m, sde, G, timesteps, n_steps, dt, x, x0_obs, mask_u8, mask_per_series, feat_std, fourier,
                                     z_steps, zobs_steps, seed, offset, B, 1, mode, stream);
}
