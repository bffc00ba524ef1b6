// fd_cfg.hip -- class-conditional score models and classifier-free guidance (Ho & Salimans 2022).  NOT in the reference, whose
// ScoreModule drops the label its datamodule reads (src/fdiff/models/score_models.py:67-94 never touches batch.y).
//
// A labelled model owns one more tensor, class_encoder.weight (K + 1, D), row K the null (unconditional) token; k_time_embed adds
// row y_b of it to the time embedding of series b (fd_score_f32.hip), which conditions every forward and training path outside the
// persistent kernel.  Here: the label path of the ABI (fd_score_set_labels), label dropout (k_label_dropout), the class-table
// gradient (k_class_table_bwd) and guided sampling:
//   s = w s_cond + (1 - w) s_uncond                (the two products as written: w = 1 gives s_cond, w = 0 gives s_uncond, exactly)
// Guidance is an option (fd_guide, fd_loop.h) of the two plain step-by-step loops of fd_sampler.hip, not a loop of its own: the entry
// points here check their arguments, plan the guide and call the shared loop body.  The two evaluations of a step run as ONE
// forward on 2B rows -- rows [0, B) carry the labels, rows [B, 2B) the same state with the null token -- and ONE kernel then reads
// x from the conditional half and the score from both, applies the reverse-SDE step (k_cfg_sde_step here: the arithmetic, Philox
// counters and element-to-lane layout of k_sde_step over n = B T C) or the ODE / data-prediction stage (k_stage<.., PAIR>,
// fd_ode.hip), and writes the new state to both halves.  No LDS, no atomics.
#include <cmath>

#include "fd_loop.h"
#include "fd_philox.h"
#include "fd_sde.h"

namespace {

constexpr int kBlock = 256;

// out[b] = y[b] (the null token K when y is null or the label lies outside [0, K]), replaced by K with probability p: label b is
// lane b % 4 of Philox counter ctr0 + b / 4
__global__ __launch_bounds__(kBlock) void k_label_dropout(const int* __restrict__ y, int* __restrict__ out, int B, int K, float p,
                                                            uint64_t seed, uint64_t ctr0) {
    const int b = blockIdx.x * kBlock + threadIdx.x;
    if (b >= B) return;
    int v = y ? y[b] : K;
    if ((unsigned)v > (unsigned)K) v = K;
    if (p > 0.f) {
        const fd_u4 r = fd_philox4x32_10(ctr0 + (uint64_t)(b >> 2), seed);
        const int l = b & 3;
        const uint32_t rv = l == 0 ? r.x : l == 1 ? r.y : l == 2 ? r.z : r.w;
        if (fd_u01(rv) < p) v = K;
    }
    out[b] = v;
}

// dTable[k, d] (+)= sum_{b : y[b] == k} dtemb[b, d], b ascending: one workgroup per table row, a thread per column
__global__ __launch_bounds__(kBlock) void k_class_table_bwd(const int* __restrict__ y, const float* __restrict__ dtemb,
                                                              float* __restrict__ dtable, int B, int D, int accumulate) {
    const int k = blockIdx.x;
    for (int d = threadIdx.x; d < D; d += kBlock) {
        float acc = 0.f;
        for (int b = 0; b < B; ++b)
            if (y[b] == k) acc += dtemb[(size_t)b * D + d];
        float* o = dtable + (size_t)k * D + d;
        *o = accumulate ? *o + acc : acc;
    }
}

// lab[0 .. B) = y (out-of-range labels: the null token), lab[B .. 2B) = K
__global__ __launch_bounds__(kBlock) void k_cfg_labels(const int* __restrict__ y, int* __restrict__ lab, int B, int K) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= 2 * B) return;
    int v = K;
    if (i < B) {
        v = y[i];
        if ((unsigned)v > (unsigned)K) v = K;
    }
    lab[i] = v;
}

// Guided Euler-Maruyama step: x (2n) in place, score (2n); group g = elements 4g .. 4g + 3 of the conditional half and Philox counter
// offset + g, as k_sde_step.  V4 (C % 4 == 0, hence n % 4 == 0 and both halves 16-byte aligned): 16-byte accesses, one row per
// group; else scalar accesses.
template <bool V4>
__global__ __launch_bounds__(kBlock) void k_cfg_sde_step(const float* __restrict__ G, float* __restrict__ x,
                                                           const float* __restrict__ score, const float* __restrict__ zin, size_t n,
                                                           int T, int C, SdeCoef cf, float w, float omw, uint64_t seed,
                                                           uint64_t offset) {
    const size_t ngroups = (n + 3) / 4;
    for (size_t g = blockIdx.x * (size_t)kBlock + threadIdx.x; g < ngroups; g += (size_t)gridDim.x * kBlock) {
        const size_t e = g * 4;
        float z[4];
        if (!zin) fd_randn4(offset + g, seed, z);
        if (V4) {
            if (zin) {
                const float4 zv = *reinterpret_cast<const float4*>(zin + e);
                z[0] = zv.x; z[1] = zv.y; z[2] = zv.z; z[3] = zv.w;
            }
            const float4 xv = *reinterpret_cast<const float4*>(x + e);
            const float4 sc = *reinterpret_cast<const float4*>(score + e);
            const float4 su = *reinterpret_cast<const float4*>(score + n + e);
            const float Gt = G[(e / (size_t)C) % (size_t)T];
            float4 o;
            o.x = fd_sde_apply(xv.x, fd_guided(sc.x, su.x, w, omw), z[0], Gt, cf);
            o.y = fd_sde_apply(xv.y, fd_guided(sc.y, su.y, w, omw), z[1], Gt, cf);
            o.z = fd_sde_apply(xv.z, fd_guided(sc.z, su.z, w, omw), z[2], Gt, cf);
            o.w = fd_sde_apply(xv.w, fd_guided(sc.w, su.w, w, omw), z[3], Gt, cf);
            *reinterpret_cast<float4*>(x + e) = o;
            *reinterpret_cast<float4*>(x + n + e) = o;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const size_t ei = e + i;
                if (ei < n) {
                    const float zi = zin ? zin[ei] : z[i];
                    const float o = fd_sde_apply(x[ei], fd_guided(score[ei], score[n + ei], w, omw), zi, G[(ei / (size_t)C) % (size_t)T], cf);
                    x[ei] = o;
                    x[n + ei] = o;
                }
            }
        }
    }
}

int cfg_check(fd_score* m, const void* G, const void* timesteps, const void* x, int n_steps, float w, const char* who) {
    fd_ctx* ctx = m->ctx;
    FD_REQUIRE(ctx, G && timesteps && x, "%s: null pointer", who);
    FD_REQUIRE(ctx, n_steps > 0, "%s: n_steps=%d", who, n_steps);
    return fd_guide_check(m, w, who);
}

}  // namespace

// ------------------------------------------------------------------ labels
int fd_labels_check(fd_score* m, int B, const char* who) {
    if (m->labels && m->labels_B != B)
        return fd_fail(m->ctx, FD_ERR_ARG, "%s: B=%d, but labels are bound for B=%d (fd_score_set_labels)", who, B, m->labels_B);
    return fd_cov_check(m, B, who);
}

int fd_labels_prepare_train(fd_score* m, int B, uint64_t seed, uint64_t offset, hipStream_t s) {
    if (m->n_classes <= 0) return FD_OK;
    fd_ctx* ctx = m->ctx;
    if (m->y_eff_cap < B) {      // grow-only; the free synchronises, so no earlier reader is left behind
        if (m->y_eff) (void)hipFree(m->y_eff);
        m->y_eff = nullptr;
        m->y_eff_cap = 0;
        const int cap = (B + 1023) & ~1023;
        FD_HIP(ctx, hipMalloc((void**)&m->y_eff, (size_t)cap * sizeof(int)));
        m->y_eff_cap = cap;
    }
    hipLaunchKernelGGL(k_label_dropout, dim3((B + kBlock - 1) / kBlock), dim3(kBlock), 0, s, m->labels, m->y_eff, B, m->n_classes,
                       m->label_dropout, seed, offset + kLabelCtrBase);
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}

int fd_class_table_backward(fd_score* m, const float* dtemb, float* grads, int B, int accumulate, hipStream_t s) {
    if (m->n_classes <= 0) return FD_OK;
    fd_ctx* ctx = m->ctx;
    if (!m->y_eff || m->y_eff_cap < B) return fd_fail(ctx, FD_ERR_STATE, "class-table gradient: no training forward has set the labels");
    hipLaunchKernelGGL(k_class_table_bwd, dim3(m->n_classes + 1), dim3(kBlock), 0, s, (const int*)m->y_eff, dtemb, grads + m->cls_w, B,
                       m->d.d_model, accumulate ? 1 : 0);
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}

void fd_labels_destroy(fd_score* m) {
    if (m->y_eff) (void)hipFree(m->y_eff);
    m->y_eff = nullptr;
    m->y_eff_cap = 0;
}

extern "C" int fd_score_set_labels(fd_score* m, const int32_t* y, int B) {
    if (!m) return FD_ERR_ARG;
    fd_ctx* ctx = m->ctx;
    if (!y) {
        m->labels = nullptr;
        m->labels_B = 0;
        return FD_OK;
    }
    FD_REQUIRE(ctx, m->n_classes > 0, "fd_score_set_labels: the model has no class table (fd_score_create_cond with n_classes > 0)");
    FD_REQUIRE(ctx, B > 0, "fd_score_set_labels: B=%d", B);
    m->labels = y;
    m->labels_B = B;
    return FD_OK;
}

extern "C" int fd_score_get_labels(fd_score* m, const int32_t** y, int* B) {
    if (!m || !y || !B) return FD_ERR_ARG;
    *y = m->labels;
    *B = m->labels_B;
    return FD_OK;
}

extern "C" int fd_score_set_label_dropout(fd_score* m, float p) {
    if (!m) return FD_ERR_ARG;
    fd_ctx* ctx = m->ctx;
    FD_REQUIRE(ctx, p >= 0.f && p <= 1.f, "fd_score_set_label_dropout: p=%f", p);
    FD_REQUIRE(ctx, m->n_classes > 0 || p == 0.f, "fd_score_set_label_dropout: the model has no class table");
    m->label_dropout = p;
    return FD_OK;
}

extern "C" int fd_label_dropout(fd_ctx* ctx, const int32_t* y, int32_t* y_out, int B, int n_classes, float p, uint64_t seed,
                                uint64_t offset, void* stream) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, y_out && B > 0 && n_classes > 0, "fd_label_dropout: null output, B=%d or n_classes=%d", B, n_classes);
    FD_REQUIRE(ctx, p >= 0.f && p <= 1.f, "fd_label_dropout: p=%f", p);
    hipLaunchKernelGGL(k_label_dropout, dim3((B + kBlock - 1) / kBlock), dim3(kBlock), 0, (hipStream_t)stream, y, y_out, B, n_classes, p,
                       seed, offset + kLabelCtrBase);
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}

// ------------------------------------------------------------------ guided loops
fd_guide fd_guide_plan(const int* y, float w) {
    // FDIFF_CFG_FORCE_PAIR (tests): the two-evaluation form also at w = 1 and w = 0, where the combine is exact
    const bool pair = y && ((w != 1.f && w != 0.f) || getenv("FDIFF_CFG_FORCE_PAIR"));
    return fd_guide{pair, (pair || w != 0.f) ? y : nullptr, w, (float)(1.0 - (double)w)};
}

int fd_guide_check(fd_score* m, float w, const char* who) {
    fd_ctx* ctx = m->ctx;
    FD_REQUIRE(ctx, m->n_classes > 0, "%s: the model has no class table (fd_score_create_cond with n_classes > 0)", who);
    FD_REQUIRE(ctx, std::isfinite(w), "%s: the guidance scale is not finite", who);
    return FD_OK;
}

// fd_cov.hip: the pair's covariates and keep bytes
int fd_guide_begin_cov(fd_score* m, const fd_guide* g, void* own, int B, hipStream_t s);

int fd_guide_begin(fd_score* m, const fd_guide* g, void* lab, float* x, int B, hipStream_t s) {
    if (!g || !g->pair) return FD_OK;
    const size_t n = (size_t)B * m->d.max_len * m->d.n_channels;
    if (g->P > 0) {
        if (int rc = fd_guide_begin_cov(m, g, lab, B, s)) return rc;
    } else {
        hipLaunchKernelGGL(k_cfg_labels, dim3((2 * B + kBlock - 1) / kBlock), dim3(kBlock), 0, s, g->y, (int*)lab, B, m->n_classes);
    }
    FD_HIP(m->ctx, hipMemcpyAsync(x + n, x, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    return FD_OK;
}

int fd_cfg_sde_step(fd_ctx* ctx, const fd_sde_params* sde, const float* G, float* x, const float* score, const float* z, uint64_t seed,
                    uint64_t offset, double t, float dt, const fd_guide& g, int B, int T, int C, hipStream_t s) {
    const size_t n = (size_t)B * T * C;
    const SdeCoef cf = fd_sde_coef(*sde, t, dt);
    const dim3 grid(fd_grid_for((n + 3) / 4, kBlock, ctx->num_cu));
    if (C % 4 == 0)
        hipLaunchKernelGGL(k_cfg_sde_step<true>, grid, dim3(kBlock), 0, s, G, x, score, z, n, T, C, cf, g.w, g.omw, seed, offset);
    else
        hipLaunchKernelGGL(k_cfg_sde_step<false>, grid, dim3(kBlock), 0, s, G, x, score, z, n, T, C, cf, g.w, g.omw, seed, offset);
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}

extern "C" int fd_sampler_run_cfg(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps, float dt,
                                  float* x, const int32_t* y, float w, const float* z_steps, uint64_t seed, uint64_t offset, int B,
                                  int mode, void* stream) {
    if (int rc = fd_loop_check(m, sde, B, mode, "fd_sampler_run_cfg")) return rc;
    fd_ctx* ctx = m->ctx;
    if (int rc = cfg_check(m, G, timesteps, x, n_steps, w, "fd_sampler_run_cfg")) return rc;
    FD_REQUIRE(ctx, dt > 0.f, "fd_sampler_run_cfg: step size must be > 0 (sde.py:158)");
    const fd_guide g = fd_guide_plan(y, w);
    return fd_sampler_sde_loop(m, sde, G, timesteps, n_steps, dt, x, z_steps, seed, offset, B, mode, (hipStream_t)stream, &g);
}

// solver: 0 Euler, 1 Heun (fd_sampler_run_ode's grids), 2 DDIM, 3 DPM-Solver++ 2M (fd_sampler_run_dpm's)
extern "C" int fd_sampler_run_ode_cfg(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps,
                                      int solver, float* x, const int32_t* y, float w, int B, int mode, void* stream) {
    if (int rc = fd_loop_check(m, sde, B, mode, "fd_sampler_run_ode_cfg")) return rc;
    fd_ctx* ctx = m->ctx;
    if (int rc = cfg_check(m, G, timesteps, x, n_steps, w, "fd_sampler_run_ode_cfg")) return rc;
    FD_REQUIRE(ctx, solver >= 0 && solver <= 3, "fd_sampler_run_ode_cfg: solver %d (0 Euler, 1 Heun, 2 DDIM, 3 DPM-Solver++ 2M)", solver);
    const fd_guide g = fd_guide_plan(y, w);
    return fd_sampler_ode_loop(m, sde, G, timesteps, n_steps, solver, x, B, mode, (hipStream_t)stream, &g);
}
