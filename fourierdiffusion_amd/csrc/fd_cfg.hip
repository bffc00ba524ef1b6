// fd_cfg.hip -- class-conditional score models and classifier-free guidance (Ho & Salimans 2022).  NOT in the reference, whose
// ScoreModule drops the label its datamodule reads (src/fdiff/models/score_models.py:67-94 never touches batch.y).
//
// A labelled model owns one more tensor, class_encoder.weight (K + 1, D), row K the null (unconditional) token; k_time_embed adds
// row y_b of it to the time embedding of series b (fd_score_f32.hip), which conditions every forward and training path outside the
// persistent kernel.  Here: the label path of the ABI (fd_score_set_labels), label dropout (k_label_dropout), the class-table
// gradient (k_class_table_bwd) and the guided sampling loops with their fused step kernels:
//   s = w s_cond + (1 - w) s_uncond                (the two products as written: w = 1 gives s_cond, w = 0 gives s_uncond, exactly)
// The two evaluations of a step run as ONE forward on 2B rows -- rows [0, B) carry the labels, rows [B, 2B) the same state with the
// null token -- and ONE kernel then reads x from the conditional half and the score from both, applies the reverse-SDE step (the
// arithmetic, Philox counters and element-to-lane layout of k_sde_step over n = B T C) or the ODE / data-prediction stage
// (fd_mega_params.h), and writes the new state to both halves.  No LDS, no atomics.
#include <cmath>

#include "fd_ode.h"
#include "fd_philox.h"
#include "fd_score.h"
#include "fd_sde.h"

namespace {

constexpr int kBlock = 256;

inline int grid_for(size_t items, int num_cu) {
    size_t blocks = (items + kBlock - 1) / kBlock;
    const size_t cap = (size_t)num_cu * 64;
    if (blocks > cap) blocks = cap;
    return (int)(blocks < 1 ? 1 : blocks);
}

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

// the guided score of one element; the intrinsics keep the two products and the sum from being contracted into an fma
__device__ __forceinline__ float guided(float sc, float su, float w, float omw) {
    return __fadd_rn(__fmul_rn(w, sc), __fmul_rn(omw, su));
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
            o.x = fd_sde_apply(xv.x, guided(sc.x, su.x, w, omw), z[0], Gt, cf);
            o.y = fd_sde_apply(xv.y, guided(sc.y, su.y, w, omw), z[1], Gt, cf);
            o.z = fd_sde_apply(xv.z, guided(sc.z, su.z, w, omw), z[2], Gt, cf);
            o.w = fd_sde_apply(xv.w, guided(sc.w, su.w, w, omw), z[3], Gt, cf);
            *reinterpret_cast<float4*>(x + e) = o;
            *reinterpret_cast<float4*>(x + n + e) = o;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const size_t ei = e + i;
                if (ei < n) {
                    const float zi = zin ? zin[ei] : z[i];
                    const float o = fd_sde_apply(x[ei], guided(score[ei], score[n + ei], w, omw), zi, G[(ei / (size_t)C) % (size_t)T], cf);
                    x[ei] = o;
                    x[n + ei] = o;
                }
            }
        }
    }
}

// Guided ODE / data-prediction stage: ownership and arithmetic of k_ode_stage / k_dpm_stage (fd_ode.hip) on the conditional half,
// the solver state x0 / v0 (B,T,C) as there; the new state goes to both halves
template <bool V4, bool DPM>
__global__ __launch_bounds__(kBlock) void k_cfg_ode_stage(const float* __restrict__ G, float* __restrict__ x,
                                                            const float* __restrict__ score, float* __restrict__ x0,
                                                            float* __restrict__ v0, size_t n, int T, int C, fd_ode_step_coef c,
                                                            fd_dpm_coef dw, float w, float omw) {
    const size_t items = V4 ? n / 4 : n;
    for (size_t i = blockIdx.x * (size_t)kBlock + threadIdx.x; i < items; i += (size_t)gridDim.x * kBlock) {
        if (V4) {
            const size_t e = 4 * i;
            const float gk = c.g * G[(e / (size_t)C) % (size_t)T];
            const float4 xv = *reinterpret_cast<const float4*>(x + e);
            const float4 sc = *reinterpret_cast<const float4*>(score + e);
            const float4 su = *reinterpret_cast<const float4*>(score + n + e);
            const float s0 = guided(sc.x, su.x, w, omw), s1 = guided(sc.y, su.y, w, omw), s2 = guided(sc.z, su.z, w, omw),
                        s3 = guided(sc.w, su.w, w, omw);
            const float4 o = DPM ? fd_dpm_stage4(xv, s0, s1, s2, s3, gk, c, dw, x0 + e) : fd_ode_stage4(xv, s0, s1, s2, s3, gk, c, x0 + e, v0 + e);
            *reinterpret_cast<float4*>(x + e) = o;
            *reinterpret_cast<float4*>(x + n + e) = o;
        } else {
            const float gk = c.g * G[(i / (size_t)C) % (size_t)T];
            const float s = guided(score[i], score[n + i], w, omw);
            const float o = DPM ? fd_dpm_stage1(x[i], s, gk, c, dw, x0 + i) : fd_ode_stage1(x[i], s, gk, c, x0 + i, v0 + i);
            x[i] = o;
            x[n + i] = o;
        }
    }
}

// What a guided loop runs: pair = two evaluations per step as one forward on 2B rows; else one evaluation on B rows with `bound`
// labels (y, or null = the null token on every row)
struct CfgPlan {
    bool pair;
    const int* bound;
};
CfgPlan cfg_plan(const int* y, float w) {
    // FDIFF_CFG_FORCE_PAIR (tests): the two-evaluation form also at w = 1 and w = 0, where the combine is exact
    const bool pair = y && ((w != 1.f && w != 0.f) || getenv("FDIFF_CFG_FORCE_PAIR"));
    return CfgPlan{pair, (!pair && y && w != 0.f) ? y : nullptr};
}

int cfg_check(fd_score* m, const void* G, const void* timesteps, const void* x, int n_steps, float w, const char* who) {
    fd_ctx* ctx = m->ctx;
    FD_REQUIRE(ctx, G && timesteps && x, "%s: null pointer", who);
    FD_REQUIRE(ctx, n_steps > 0, "%s: n_steps=%d", who, n_steps);
    FD_REQUIRE(ctx, m->n_classes > 0, "%s: the model has no class table (fd_score_create_cond with n_classes > 0)", who);
    FD_REQUIRE(ctx, std::isfinite(w), "%s: the guidance scale is not finite", who);
    return FD_OK;
}

// binds the loop's own label vector for its forwards; the caller's binding is back when the scope ends (the kernels have taken their
// pointers at launch)
struct LabelScope {
    fd_score* m;
    const int* y;
    int B;
    LabelScope(fd_score* mm, const int* lab, int rows) : m(mm), y(mm->labels), B(mm->labels_B) {
        m->labels = lab;
        m->labels_B = lab ? rows : 0;
    }
    ~LabelScope() {
        m->labels = y;
        m->labels_B = B;
    }
};

}  // namespace

// ------------------------------------------------------------------ labels
int fd_labels_check(fd_score* m, int B, const char* who) {
    if (m->labels && m->labels_B != B)
        return fd_fail(m->ctx, FD_ERR_ARG, "%s: B=%d, but labels are bound for B=%d (fd_score_set_labels)", who, B, m->labels_B);
    return FD_OK;
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
// Workspace of a guided loop behind the forward scratch of R rows: score (R,T,C), nstate solver buffers (B,T,C), labels (2B) when
// pair; then fd_step_table's t vectors.
extern "C" int fd_sampler_run_cfg(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps, float dt,
                                  float* x, const int32_t* y, float w, const float* z_steps, uint64_t seed, uint64_t offset, int B,
                                  int mode, void* stream) {
    if (int rc = fd_loop_check(m, sde, B, mode, "fd_sampler_run_cfg")) return rc;
    fd_ctx* ctx = m->ctx;
    if (int rc = cfg_check(m, G, timesteps, x, n_steps, w, "fd_sampler_run_cfg")) return rc;
    FD_REQUIRE(ctx, dt > 0.f, "fd_sampler_run_cfg: step size must be > 0 (sde.py:158)");
    hipStream_t s = (hipStream_t)stream;
    const CfgPlan pl = cfg_plan(y, w);
    const int T = m->d.max_len, C = m->d.n_channels, K = m->n_classes;
    const int R = pl.pair ? 2 * B : B;
    const size_t n = (size_t)B * T * C;
    const size_t fwd = fd_loop_fwd_workspace(m, R);
    const size_t sbytes = fd_ws::padded((size_t)R * T * C * sizeof(float));
    const size_t lbytes = pl.pair ? fd_ws::padded((size_t)R * sizeof(int)) : 0;
    float* tvec0 = nullptr;
    size_t tstride = 0;
    if (int rc = fd_step_table(ctx, fwd, sbytes + lbytes, timesteps, n_steps, R, s, &tvec0, &tstride)) return rc;
    float* score = (float*)((char*)ctx->ws + fwd);
    int* lab = (int*)((char*)ctx->ws + fwd + sbytes);
    if (pl.pair) {
        hipLaunchKernelGGL(k_cfg_labels, dim3((R + kBlock - 1) / kBlock), dim3(kBlock), 0, s, y, lab, B, K);
        FD_HIP(ctx, hipMemcpyAsync(x + n, x, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    LabelScope scope(m, pl.pair ? lab : pl.bound, R);
    const float omw = (float)(1.0 - (double)w);
    const uint64_t per_step = (uint64_t)((n + 3) / 4);
    for (int i = 0; i < n_steps; ++i) {
        float* tvec = tvec0 + (size_t)i * tstride;
        if (!tstride) fd_fill(tvec, R, timesteps[i], s);
        if (int rc = fd_score_forward_any(m, x, tvec, score, R, mode, s)) return rc;
        const float* z = z_steps ? z_steps + (size_t)i * n : nullptr;
        const uint64_t ctr = offset + (uint64_t)i * per_step;
        if (!pl.pair) {
            if (int rc = fd_sde_step(ctx, sde, G, x, score, z, seed, ctr, (double)timesteps[i], dt, x, B, T, C, stream)) return rc;
            continue;
        }
        const SdeCoef cf = fd_sde_coef(*sde, (double)timesteps[i], dt);
        if (C % 4 == 0)
            hipLaunchKernelGGL(k_cfg_sde_step<true>, dim3(grid_for(per_step, ctx->num_cu)), dim3(kBlock), 0, s, G, x, (const float*)score, z,
                               n, T, C, cf, w, omw, seed, ctr);
        else
            hipLaunchKernelGGL(k_cfg_sde_step<false>, dim3(grid_for(per_step, ctx->num_cu)), dim3(kBlock), 0, s, G, x, (const float*)score, z,
                               n, T, C, cf, w, omw, seed, ctr);
    }
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}

// solver: 0 Euler, 1 Heun (fd_sampler_run_ode's grids), 2 DDIM, 3 DPM-Solver++ 2M (fd_sampler_run_dpm's)
extern "C" int fd_sampler_run_ode_cfg(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps,
                                      int solver, float* x, const int32_t* y, float w, int B, int mode, void* stream) {
    if (int rc = fd_loop_check(m, sde, B, mode, "fd_sampler_run_ode_cfg")) return rc;
    fd_ctx* ctx = m->ctx;
    if (int rc = cfg_check(m, G, timesteps, x, n_steps, w, "fd_sampler_run_ode_cfg")) return rc;
    FD_REQUIRE(ctx, solver >= 0 && solver <= 3, "fd_sampler_run_ode_cfg: solver %d (0 Euler, 1 Heun, 2 DDIM, 3 DPM-Solver++ 2M)", solver);
    std::vector<fd_ode_step_coef> rows;
    std::vector<fd_dpm_coef> dpm;
    const bool is_dpm = solver >= 2;
    if (is_dpm) {
        if (int rc = fd_dpm_table(ctx, sde, timesteps, n_steps, solver, &rows, &dpm)) return rc;
    } else if (int rc = fd_ode_table(ctx, sde, timesteps, n_steps, solver, &rows)) {
        return rc;
    }
    const int nstate = solver == 1 ? 2 : solver == 3 ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    const CfgPlan pl = cfg_plan(y, w);
    const int T = m->d.max_len, C = m->d.n_channels, K = m->n_classes;
    const int R = pl.pair ? 2 * B : B;
    const int n_eval = (int)rows.size();
    const size_t n = (size_t)B * T * C;
    const size_t fwd = fd_loop_fwd_workspace(m, R);
    const size_t sbytes = fd_ws::padded((size_t)R * T * C * sizeof(float));
    const size_t buf = fd_ws::padded(n * sizeof(float));
    const size_t lbytes = pl.pair ? fd_ws::padded((size_t)R * sizeof(int)) : 0;
    std::vector<float> t_eval(n_eval);
    for (int k = 0; k < n_eval; ++k) t_eval[k] = rows[k].t;
    float* tvec0 = nullptr;
    size_t tstride = 0;
    if (int rc = fd_step_table(ctx, fwd, sbytes + nstate * buf + lbytes, t_eval.data(), n_eval, R, s, &tvec0, &tstride)) return rc;
    char* base = (char*)ctx->ws + fwd;
    float* score = (float*)base;
    float* x0 = nstate > 0 ? (float*)(base + sbytes) : nullptr;
    float* v0 = nstate > 1 ? (float*)(base + sbytes + buf) : nullptr;
    int* lab = (int*)(base + sbytes + nstate * buf);
    if (pl.pair) {
        hipLaunchKernelGGL(k_cfg_labels, dim3((R + kBlock - 1) / kBlock), dim3(kBlock), 0, s, y, lab, B, K);
        FD_HIP(ctx, hipMemcpyAsync(x + n, x, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    LabelScope scope(m, pl.pair ? lab : pl.bound, R);
    const float omw = (float)(1.0 - (double)w);
    const bool v4 = C % 4 == 0;
    const int grid = grid_for(v4 ? n / 4 : n, ctx->num_cu);
    for (int k = 0; k < n_eval; ++k) {
        float* tvec = tvec0 + (size_t)k * tstride;
        if (!tstride) fd_fill(tvec, R, t_eval[k], s);
        if (int rc = fd_score_forward_any(m, x, tvec, score, R, mode, s)) return rc;
        if (!pl.pair) {
            if (int rc = fd_ode_stage(ctx, G, x, score, x0, v0, rows[k], B, T, C, s, is_dpm ? &dpm[k] : nullptr)) return rc;
            continue;
        }
        const fd_dpm_coef dw = is_dpm ? dpm[k] : fd_dpm_coef{};
#define FD_CFG_ODE(V4_, DPM_)                                                                                                         \
    hipLaunchKernelGGL((k_cfg_ode_stage<V4_, DPM_>), dim3(grid), dim3(kBlock), 0, s, G, x, (const float*)score, x0, v0, n, T, C, rows[k], \
                       dw, w, omw)
        if (v4 && is_dpm) FD_CFG_ODE(true, true);
        else if (v4) FD_CFG_ODE(true, false);
        else if (is_dpm) FD_CFG_ODE(false, true);
        else FD_CFG_ODE(false, false);
#undef FD_CFG_ODE
    }
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}
