// fd_smc.hip -- twisted sequential Monte Carlo conditioning: the Twisted Diffusion Sampler (Wu et al., NeurIPS 2023) around the
// guidance evaluation of fd_dps.hip, NOT in the reference.  A series is carried by K adjacent state rows (particles) that read its
// observation in place (obs_replicas = K).  The observation model is y = A(x_0) + obs_std eps at the observed entries (data scale,
// time domain).  Per row and step t_i -> t_{i+1}, (alpha_i, s_i) the perturbation kernel at t_i, rho_i = ||r||^2 and
// g_i = -grad_x rho_i of fd_dps.hip, cf the coefficients of fd_sde_apply, per element n = sqrt(dt) g(t_i) G_k z the step's noise
// term and S = dt g(t_i)^2 G_k^2 its variance:
//
//   v_i      = obs_std^2 + twist_scale (s_i / alpha_i)^2                     twist variance (any v_i > 0 is consistent)
//   ltw_i(x) = -rho_i(x) / (2 v_i)                                           log twist, unnormalised
//   h_i      = g_i / (2 v_i)                                                 = grad_x ltw_i (exact with the Jacobian)
//   x_{i+1}  = fd_sde_apply(x_i, score_i, z_i) + S . h_i                     proposal (term skipped where h == 0, as k_dps_step)
//   c1 = sum_e n_e h_e,  c2 = sum_e S_e h_e^2                                per row
//   logw    += -c1 - c2 / 2 + ltw_{i+1}(x_{i+1}) - ltw_i(x_i)                log p/q of the step + twist ratio
//
// x_0 is the prior's and logw = ltw_0(x_0).  After the last step the twist is the likelihood itself: rho_N is the residual of x_N
// with alpha = 1, s = 0 (no network evaluation) and v_N = obs_std^2.  Stage j = 0 .. N runs after evaluation j and before step j
// (stage N is the final one), per series over its K rows, in double: W = softmax(logw) (a NaN or infinite logw is weight 0),
// ESS = 1 / sum W^2; if ESS < ess_threshold K (or always at stage N under final_resample): logZ += logsumexp(logw) - log K,
// systematic resampling with ONE uniform u per (stage, series), a[k] = min{j : cumW[j] > (u + k) / K} clamped to K - 1, logw = 0;
// else logw is kept.  Stage N resamples under final_resample alone (without it never: the weighted rows are returned and their
// logsumexp - log K still goes to the evidence).  A series whose particles all have weight 0 is not resampled, evidence -inf.
//
// k_smc_weights: one workgroup per series, thread k = particle k.  Finishes the logw update from the residual's block sums, the
// step's chunk sums and the stored ltw, each summed in index order, then the stage: wave scan (shuffles), then the waves in order
// through the LDS, so every sum has one order.  Writes the ancestors, the ltw permuted to the new rows, the stage's trace and the
// logZ increment; the decision to resample never leaves the device.
// k_smc_step: one workgroup per (row, chunk of 1024 elements), a thread per 4 consecutive elements OF THE ROW, noise from the
// Philox groups of k_sde_step (element e of the (B,T,C) tensor is lane e % 4 of counter offset + e / 4; a row that does not start on
// a group boundary evaluates the two groups it straddles).  Reads x, score, u, dx through the ancestor index and writes the other
// state buffer, so resampling costs no pass of its own; c1 and c2 leave as one double pair per (row, chunk) from a fixed-order LDS
// tree over partial sums that depend on the row's own elements alone: bit-reproducible and independent of the launch's other rows.
// The file is built with the library's flags (-fno-honor-nans, as fd_dps.hip, so that fd_sde_apply compiles here as it does there):
// the stage finds a non-finite log weight by its exponent bits and replaces it by -inf before any arithmetic sees it.
#include <algorithm>
#include <cmath>
#include <vector>

#include "fd_common.h"
#include "fd_dps.h"
#include "fd_engine.h"
#include "fd_loop.h"
#include "fd_philox.h"
#include "fd_sde.h"

namespace {

constexpr int kStepBlock = 256;              // k_smc_step: threads per workgroup
constexpr int kChunk = 4 * kStepBlock;       // elements of one row per workgroup
constexpr int kMaxK = 1024;                  // particles per series = threads of k_smc_weights
constexpr int kMaxWaves = kMaxK / 64;

struct SmcStepArgs {
    const float* G;
    const float* x;          // (B,T,C) state x_i, rows before the stage's resampling
    const float* score;
    const float* u;          // with dx: g = (2 / alpha) (u + dx), as k_dps_step
    const float* dx;         // or nullptr
    const float* g;          // g given (fd_smc_step) instead of u, dx
    const float* zin;        // injected predictor noise (B,T,C) of the NEW rows, or nullptr (Philox at offset)
    const int* anc;          // (B) ancestor inside the series, or nullptr (identity)
    float* xout;             // (B,T,C) the other state buffer
    double* c1p;             // (B, nch)
    double* c2p;
    size_t TC;
    int T, C, K, nch;
    SdeCoef cf;
    float alpha, inv2v;
    uint64_t seed, offset;
};

// fd_sde_apply with the contraction k_dps_step compiles it to, written out: drift = fma(x, -a_x, -(s gk^2)), x' = fma(sqrt_dt, gk z,
// fma(-dt, drift, x)).  Inlined next to the proposal's own products the compiler packs fd_sde_apply's multiplies (v_pk_mul_f32) and
// contracts them differently, and an all-false mask would no longer give that kernel's bits (tests/test_gpu_smc.py holds the two equal)
__device__ __forceinline__ float smc_sde_apply(float x, float s, float z, float gk, const SdeCoef& cf) {
    const float drift = __fmaf_rn(x, -cf.a_x, -__fmul_rn(s, __fmul_rn(gk, gk)));
    return __fmaf_rn(cf.sqrt_dt, __fmul_rn(z, gk), __fmaf_rn(-cf.dt, drift, x));
}

__global__ __launch_bounds__(kStepBlock) void k_smc_step(SmcStepArgs a) {
    __shared__ double red1[kStepBlock];
    __shared__ double red2[kStepBlock];
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x / a.nch;
    const int ch = blockIdx.x % a.nch;
    size_t src = b;
    if (a.anc) {
        const int k = min(max(a.anc[b], 0), a.K - 1);
        src = b / a.K * a.K + k;
    }
    const size_t base = b * a.TC, sbase = src * a.TC;
    const size_t loc0 = (size_t)ch * kChunk + 4 * (size_t)tid;
    double s1 = 0.0, s2 = 0.0;
    if (loc0 < a.TC) {
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        if (a.zin) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (loc0 + j < a.TC) z[j] = a.zin[base + loc0 + j];
        } else {
            const size_t e0 = base + loc0;
            const int r = (int)(e0 & 3);
            float zz[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            float za[4], zb[4];
            fd_randn4(a.offset + (e0 >> 2), a.seed, za);
#pragma unroll
            for (int j = 0; j < 4; ++j) zz[j] = za[j];
            if (r != 0) {      // (uniform over the workgroup: base and the chunk decide it)
                fd_randn4(a.offset + (e0 >> 2) + 1, a.seed, zb);
#pragma unroll
                for (int j = 0; j < 4; ++j) zz[4 + j] = zb[j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (k == r + j) z[j] = zz[k];
        }
        const float tw = 2.0f / a.alpha;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const size_t loc = loc0 + j;
            if (loc >= a.TC) break;
            const size_t es = sbase + loc;
            const int t = (int)(loc / a.C);
            const float Gt = a.G[t];
            float gv;
            if (a.g) gv = a.g[es];
            else gv = tw * (a.u[es] + (a.dx ? a.dx[es] : 0.f));
            const float h = gv * a.inv2v;
            const float gk = __fmul_rn(a.cf.g, Gt);
            float xv = smc_sde_apply(a.x[es], a.score[es], z[j], gk, a.cf);
            const float S = a.cf.dt * (gk * gk);
            if (h != 0.f) xv += S * h;
            a.xout[base + loc] = xv;
            const double nd = (double)a.cf.sqrt_dt * ((double)gk * (double)z[j]);
            s1 += nd * (double)h;
            s2 += (double)S * ((double)h * (double)h);
        }
    }
    red1[tid] = s1;
    red2[tid] = s2;
    __syncthreads();
#pragma unroll
    for (int w = kStepBlock / 2; w > 0; w >>= 1) {
        if (tid < w) {
            red1[tid] += red1[tid + w];
            red2[tid] += red2[tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        a.c1p[blockIdx.x] = red1[0];
        a.c2p[blockIdx.x] = red2[0];
    }
}

// out[b] = sum_c part[b][c], c ascending
__global__ void k_smc_rowsum(const double* p1, const double* p2, double* o1, double* o2, int B, int nch) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double s1 = 0.0, s2 = 0.0;
    for (int c = 0; c < nch; ++c) {
        s1 += p1[(size_t)b * nch + c];
        s2 += p2[(size_t)b * nch + c];
    }
    o1[b] = s1;
    o2[b] = s2;
}

// out row b = in row (ancestor of b): the final stage's resampling, into the caller's buffer
__global__ __launch_bounds__(256) void k_smc_gather(const float* in, const int* anc, float* out, size_t n, size_t TC, int K) {
    for (size_t e = blockIdx.x * (size_t)256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        const size_t b = e / TC, loc = e - b * TC;
        const int k = min(max(anc[b], 0), K - 1);
        out[e] = in[(b / K * K + k) * TC + loc];
    }
}

struct SmcWArgs {
    double* logw;            // (B) in / out
    const double* part;      // (B, ncb) block sums of rho at the new state, or nullptr: logw as given (fd_smc_resample)
    const double* c1p;       // (B, nch) of the step that made the state, or nullptr (stage 0)
    const double* c2p;
    double* ltw;             // (B): in, the log twist the rows left with (read unless first); out, this stage's, permuted
    int* anc;                // (B)
    const double* u_in;      // (n) this stage's uniforms, or nullptr: Philox word uidx0 + series
    double* logz;            // (n) running evidence, or nullptr
    double* dlogz_out;       // (n) this stage's increment, or nullptr
    double* ess_out;         // (n) or nullptr
    uint8_t* res_out;        // (n) or nullptr
    int* anc_out;            // (B) or nullptr
    double inv2v, thr;
    uint64_t seed, uoffset, uidx0;
    int K, ncb, nch, first, force, final_stage;
};

// inclusive scan of v over the workgroup: Hillis-Steele inside a wave, then the waves before this one added in order; *total = the
// sum of all waves in order.  sh: kMaxWaves doubles, free again when the call returns
__device__ __forceinline__ double block_scan(double v, double* sh, int lane, int wave, int nwave, double* total) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    __syncthreads();
    if (lane == 63) sh[wave] = v;
    __syncthreads();
    double before = 0.0, all = 0.0;
    for (int w = 0; w < nwave; ++w) {
        if (w == wave) before = all;
        all += sh[w];
    }
    *total = all;
    return before + v;
}

__global__ __launch_bounds__(kMaxK) void k_smc_weights(SmcWArgs a) {
    __shared__ double sh[kMaxWaves];
    __shared__ double cum[kMaxK];
    __shared__ double ltws[kMaxK];
    const int k = threadIdx.x, lane = k & 63, wave = k >> 6, nwave = blockDim.x >> 6;
    const int K = a.K, sidx = blockIdx.x;
    const size_t b = (size_t)sidx * K + k;
    const bool live = k < K;
    double lw = -INFINITY, ltw = 0.0;
    if (live) {
        lw = a.first ? 0.0 : a.logw[b];
        if (a.part) {
            if (a.c1p) {
                double c1 = 0.0, c2 = 0.0;
                for (int c = 0; c < a.nch; ++c) {
                    c1 += a.c1p[b * a.nch + c];
                    c2 += a.c2p[b * a.nch + c];
                }
                lw += -c1 - 0.5 * c2;
            }
            double rho = 0.0;
            for (int c = 0; c < a.ncb; ++c) rho += a.part[b * a.ncb + c];
            ltw = -rho * a.inv2v;
            lw += a.first ? ltw : ltw - a.ltw[b];
        }
    }
    // (exponent bits all ones: NaN or +-inf; an integer test, which no floating-point flag can fold away)
    const bool valid = live && ((unsigned long long)__double_as_longlong(lw) >> 52 & 0x7ffull) != 0x7ffull;
    // the maximum (order-free)
    double m = valid ? lw : -INFINITY;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) m = fmax(m, __shfl_xor(m, d, 64));
    if (lane == 0) sh[wave] = m;
    __syncthreads();
    m = sh[0];
    for (int w = 1; w < nwave; ++w) m = fmax(m, sh[w]);
    const double logK = log((double)K);
    if (!(m > -INFINITY)) {      // every particle has weight 0: nothing to resample from
        if (live) {
            a.logw[b] = lw;
            if (a.ltw) a.ltw[b] = ltw;
            a.anc[b] = k;
            if (a.anc_out) a.anc_out[b] = k;
        }
        if (k == 0) {
            if (a.logz) a.logz[sidx] = -INFINITY;
            if (a.dlogz_out) a.dlogz_out[sidx] = -INFINITY;
            if (a.ess_out) a.ess_out[sidx] = 0.0;
            if (a.res_out) a.res_out[sidx] = 0;
        }
        return;
    }
    const double w = valid ? exp(lw - m) : 0.0;
    double tot, sq, one;
    (void)block_scan(w, sh, lane, wave, nwave, &tot);
    const double Wn = w / tot;
    (void)block_scan(Wn * Wn, sh, lane, wave, nwave, &sq);
    const double cw = block_scan(Wn, sh, lane, wave, nwave, &one);
    const double ess = 1.0 / sq;
    const bool resample = a.force || ess < a.thr * (double)K;
    const double inc = (resample || a.final_stage) ? m + log(tot) - logK : 0.0;
    int anc = k;
    if (resample) {
        cum[k] = live ? cw : INFINITY;
        ltws[k] = ltw;
        __syncthreads();
        double u;
        if (a.u_in) {
            u = a.u_in[sidx];
        } else {
            const uint64_t idx = a.uidx0 + (uint64_t)sidx;
            const fd_u4 r = fd_philox4x32_10(a.uoffset + (idx >> 2), a.seed);
            const uint32_t word = (idx & 3) == 0 ? r.x : (idx & 3) == 1 ? r.y : (idx & 3) == 2 ? r.z : r.w;
            u = (double)fd_u01(word);
        }
        const double target = (u + (double)k) / (double)K;
        int lo = 0, hi = K - 1;      // the first j with cum[j] > target, K - 1 when there is none
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cum[mid] > target) hi = mid;
            else lo = mid + 1;
        }
        anc = lo;
        lw = 0.0;
        ltw = ltws[anc];
    }
    if (live) {
        a.logw[b] = lw;
        if (a.ltw) a.ltw[b] = ltw;
        a.anc[b] = anc;
        if (a.anc_out) a.anc_out[b] = anc;
    }
    if (k == 0) {
        if (a.logz) a.logz[sidx] += inc;
        if (a.dlogz_out) a.dlogz_out[sidx] = inc;
        if (a.ess_out) a.ess_out[sidx] = ess;
        if (a.res_out) a.res_out[sidx] = resample ? 1 : 0;
    }
}

int check_particles(fd_ctx* ctx, int B, int particles, const char* who) {
    FD_REQUIRE(ctx, particles >= 2 && particles <= kMaxK, "%s: particles=%d must lie in [2, %d]", who, particles, kMaxK);
    FD_REQUIRE(ctx, B > 0 && B % particles == 0, "%s: B=%d is not a positive multiple of particles=%d", who, B, particles);
    return FD_OK;
}

int launch_weights(fd_ctx* ctx, const SmcWArgs& a, int n, hipStream_t s) {
    const int threads = (a.K + 63) / 64 * 64;
    hipLaunchKernelGGL(k_smc_weights, dim3((unsigned)n), dim3(threads), 0, s, a);
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}

int launch_step(fd_ctx* ctx, const SmcStepArgs& a, int B, hipStream_t s) {
    hipLaunchKernelGGL(k_smc_step, dim3((unsigned)((size_t)B * a.nch)), dim3(kStepBlock), 0, s, a);
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}

}  // namespace

extern "C" int fd_smc_resample(fd_ctx* ctx, double* logw, const double* u, int n, int particles, double ess_threshold, int force,
                               int final_stage, int32_t* ancestors, double* ess, uint8_t* resampled, double* dlogz, void* stream) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, logw && u && ancestors, "fd_smc_resample: null pointer");
    FD_REQUIRE(ctx, n > 0 && n <= (1 << 24), "fd_smc_resample: n=%d", n);
    FD_REQUIRE(ctx, particles >= 2 && particles <= kMaxK, "fd_smc_resample: particles=%d must lie in [2, %d]", particles, kMaxK);
    FD_REQUIRE(ctx, ess_threshold >= 0.0 && ess_threshold <= 1.0, "fd_smc_resample: ess_threshold=%g must lie in [0, 1]",
               ess_threshold);
    SmcWArgs a{};
    a.logw = logw; a.anc = ancestors; a.u_in = u;
    a.dlogz_out = dlogz; a.ess_out = ess; a.res_out = resampled;
    a.thr = ess_threshold;
    a.K = particles; a.force = force != 0; a.final_stage = final_stage != 0;
    return launch_weights(ctx, a, n, (hipStream_t)stream);
}

extern "C" int fd_smc_step(fd_ctx* ctx, const fd_sde_params* sde, const float* G, double t, float dt, const float* x,
                           const float* score, const float* g, const int32_t* ancestors, const float* z, uint64_t seed,
                           uint64_t offset, double inv2v, float* x_out, double* c1, double* c2, int B, int particles, int T, int C,
                           void* stream) {
    if (!ctx) return FD_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    FD_REQUIRE(ctx, sde && G && x && score && g && x_out && c1 && c2, "fd_smc_step: null pointer");
    FD_REQUIRE(ctx, sde->kind == 0 || sde->kind == 1, "fd_smc_step: unknown SDE kind %d", sde->kind);
    FD_REQUIRE(ctx, dt > 0.f, "fd_smc_step: step size must be > 0");
    FD_REQUIRE(ctx, T > 0 && C > 0, "fd_smc_step: T=%d C=%d", T, C);
    FD_REQUIRE(ctx, std::isfinite(inv2v) && inv2v >= 0.0, "fd_smc_step: inv2v=%g must be finite and >= 0", inv2v);
    FD_REQUIRE(ctx, x != x_out, "fd_smc_step: x_out must not be x (rows are read through the ancestors)");
    if (int rc = check_particles(ctx, B, particles, "fd_smc_step")) return rc;
    SmcStepArgs a{};
    a.TC = (size_t)T * C;
    a.nch = (int)((a.TC + kChunk - 1) / kChunk);
    FD_REQUIRE(ctx, (long long)B * a.nch < (1ll << 31), "fd_smc_step: B=%d too large for one launch", B);
    const size_t np = (size_t)B * a.nch;
    if (int rc = fd_ll_carve(ctx, [&](auto take) {
            a.c1p = (double*)take(np * sizeof(double));
            a.c2p = (double*)take(np * sizeof(double));
        }))
        return rc;
    a.G = G; a.x = x; a.score = score; a.g = g; a.zin = z; a.anc = ancestors; a.xout = x_out;
    a.T = T; a.C = C; a.K = particles;
    a.cf = fd_sde_coef(*sde, t, dt);
    a.alpha = 1.f;
    a.inv2v = (float)inv2v;
    a.seed = seed; a.offset = offset;
    if (int rc = launch_step(ctx, a, B, s)) return rc;
    hipLaunchKernelGGL(k_smc_rowsum, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, a.c1p, a.c2p, c1, c2, B, a.nch);
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}

extern "C" int fd_sampler_run_impute_smc(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps,
                                         float dt, float* x, const float* x0_obs, const uint8_t* mask_u8, int mask_per_series,
                                         const float* feat_std, int fourier, int jacobian, double obs_std, double twist_scale,
                                         double ess_threshold, int final_resample, const float* z_steps, const double* u_stages,
                                         uint64_t seed, uint64_t offset, int B, int particles, int mode, double* log_evidence,
                                         double* log_weights, double* ess, uint8_t* resampled, int32_t* ancestors, void* stream) {
    const char* who = "fd_sampler_run_impute_smc";
    if (int rc = fd_loop_check(m, sde, B, mode, who)) return rc;
    fd_ctx* ctx = m->ctx;
    hipStream_t s = (hipStream_t)stream;
    FD_REQUIRE(ctx, timesteps, "%s: null pointer", who);
    FD_REQUIRE(ctx, n_steps > 0, "%s: n_steps=%d", who, n_steps);
    FD_REQUIRE(ctx, dt > 0.f, "%s: step size must be > 0 (sde.py:158)", who);
    if (int rc = check_particles(ctx, B, particles, who)) return rc;
    FD_REQUIRE(ctx, std::isfinite(obs_std) && obs_std > 0.0, "%s: obs_std=%g must be finite and > 0", who, obs_std);
    FD_REQUIRE(ctx, ess_threshold >= 0.0 && ess_threshold <= 1.0, "%s: ess_threshold=%g must lie in [0, 1]", who, ess_threshold);
    FD_REQUIRE(ctx, std::isfinite(twist_scale) && twist_scale >= 0.0, "%s: twist_scale=%g must be finite and >= 0", who, twist_scale);
    fd_dps_res r{};
    if (int rc = fd_dps_prepare(m, r, G, x, x0_obs, mask_u8, mask_per_series, feat_std, fourier, B, particles, s, who)) return rc;
    const bool jac = jacobian != 0;
    const int K = particles, nser = B / K, N = n_steps;
    const size_t TC = (size_t)r.T * r.C, n = (size_t)B * TC;
    const int nch = (int)((TC + kChunk - 1) / kChunk);
    FD_REQUIRE(ctx, (long long)B * nch < (1ll << 31), "%s: B=%d too large for one launch", who, B);
    fd_dps_bufs bf;
    float* xs[2];
    double *logw, *ltw, *c1p, *c2p, *logz;
    int* anc;
    if (int rc = fd_ll_carve(ctx, [&](auto take) {
            fd_dps_take(take, B, B, n, r.ncb, jac, false, &bf);
            xs[0] = (float*)take(n * sizeof(float));
            xs[1] = (float*)take(n * sizeof(float));
            logw = (double*)take((size_t)B * sizeof(double));
            ltw = (double*)take((size_t)B * sizeof(double));
            c1p = (double*)take((size_t)B * nch * sizeof(double));
            c2p = (double*)take((size_t)B * nch * sizeof(double));
            logz = (double*)take((size_t)nser * sizeof(double));
            anc = (int*)take((size_t)B * sizeof(int));
        }))
        return rc;
    r.u = bf.u; r.dout = bf.dout; r.part = bf.part;
    // per-step coefficients on the host up front: the SDE step's, Tweedie's (alpha, s) at t_i, and 1 / (2 v_i) of the twist
    std::vector<SdeCoef> cf(N);
    std::vector<float> al(N), s2(N);
    std::vector<double> inv2v(N + 1);
    for (int i = 0; i < N; ++i) {
        cf[i] = fd_sde_coef(*sde, (double)timesteps[i], dt);
        double aa = 1.0, ss = 0.0;
        fd_marginal_coef(*sde, (double)timesteps[i], &aa, &ss);
        al[i] = (float)aa;
        s2[i] = (float)(ss * ss);
        inv2v[i] = 1.0 / (2.0 * (obs_std * obs_std + twist_scale * (ss / aa) * (ss / aa)));
    }
    inv2v[N] = 1.0 / (2.0 * obs_std * obs_std);
    fd_train_mode_scope tm(m, jac ? fd_diff_train_mode(m, mode) : m->train_mode);
    fd_label_dropout_scope ld(m, 0.f);
    FD_HIP(ctx, hipMemsetAsync(logz, 0, (size_t)nser * sizeof(double), s));
    // Philox: predictor noise of step i at offset + i*ceil(BTC/4) (as fd_sampler_run); the uniform of (stage j, series q) is word
    // (j n + q) % 4 of counter offset + N*ceil(BTC/4) + (j n + q) / 4: behind the last predictor group
    const uint64_t per_step = (uint64_t)((n + 3) / 4);
    SmcWArgs w{};
    w.logw = logw; w.part = bf.part; w.ltw = ltw; w.anc = anc; w.logz = logz;
    w.thr = ess_threshold;
    w.seed = seed; w.uoffset = offset + (uint64_t)N * per_step;
    w.K = K; w.ncb = r.ncb; w.nch = nch;
    SmcStepArgs a{};
    a.G = G; a.score = bf.score; a.u = bf.u; a.dx = bf.dx; a.anc = anc; a.c1p = c1p; a.c2p = c2p;
    a.TC = TC; a.T = r.T; a.C = r.C; a.K = K; a.nch = nch;
    a.seed = seed;
    auto stage = [&](int j) {
        w.first = j == 0;
        w.c1p = j ? c1p : nullptr;
        w.c2p = j ? c2p : nullptr;
        w.inv2v = inv2v[j];
        w.u_in = u_stages ? u_stages + (size_t)j * nser : nullptr;
        w.uidx0 = (uint64_t)j * (uint64_t)nser;
        w.force = j == N && final_resample;
        w.thr = j == N && !final_resample ? 0.0 : ess_threshold;      // the final stage resamples under final_resample alone
        w.final_stage = j == N;
        w.ess_out = ess ? ess + (size_t)j * nser : nullptr;
        w.res_out = resampled ? resampled + (size_t)j * nser : nullptr;
        w.anc_out = ancestors ? ancestors + (size_t)j * B : nullptr;
        return launch_weights(ctx, w, nser, s);
    };
    const float* cur = x;
    for (int i = 0; i < N; ++i) {
        fd_fill(bf.tvec, B, timesteps[i], s);
        r.alpha = al[i];
        r.s2 = s2[i];
        if (int rc = fd_dps_eval(m, r, bf, cur, B, B, nullptr, jac, fourier != 0, mode, s)) return rc;
        if (int rc = stage(i)) return rc;
        a.x = cur;
        a.xout = xs[i & 1];
        a.zin = z_steps ? z_steps + (size_t)i * n : nullptr;
        a.cf = cf[i];
        a.alpha = al[i];
        a.inv2v = (float)inv2v[i];
        a.offset = offset + (uint64_t)i * per_step;
        if (int rc = launch_step(ctx, a, B, s)) return rc;
        cur = a.xout;
    }
    // the final stage: the likelihood of x_N itself (alpha = 1, s = 0: x0_hat = x, the stale score is multiplied by 0)
    r.x = cur;
    r.score = bf.score;
    r.alpha = 1.f;
    r.s2 = 0.f;
    r.dout = nullptr;
    if (int rc = fd_dps_residual(ctx, r, B, fourier != 0, s)) return rc;
    if (int rc = stage(N)) return rc;
    hipLaunchKernelGGL(k_smc_gather, dim3((unsigned)fd_grid_for(n, 256, ctx->num_cu)), dim3(256), 0, s, cur, anc, x, n, TC, K);
    FD_LAUNCH_CHECK(ctx);
    if (log_evidence) FD_HIP(ctx, hipMemcpyAsync(log_evidence, logz, (size_t)nser * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (log_weights) FD_HIP(ctx, hipMemcpyAsync(log_weights, logw, (size_t)B * sizeof(double), hipMemcpyDeviceToDevice, s));
    return FD_OK;
}
